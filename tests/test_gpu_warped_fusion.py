"""GPU checks of warped depth fusion (lsf_fusion_integrate_depth_warped in csrc/lsf_fusion.hip) against the existing
entry points where a warp field reduces to them, against the numpy restatement (tests/warped_fusion_restatement.py), past
the capped grid's first trip, and end to end on a deforming scene (tests/deforming_scene.py) with
HierarchicalOptimizer3d as SequenceFusion3d's non-rigid step.  tsdf, weight and the colour volume are compared bit for
bit, the record's counts and maximum exactly, and its float64 sum to the 1e-12 relative of tests/fusion_restatement.py."""
import functools

import numpy as np
import pytest
import torch

import deforming_scene as D
import fusion_weighted_restatement as FW
import rigid3d_restatement as R3
import warped_fusion_restatement as WR
from test_gpu_colour import BIG, BIG_OFF, CAP, FUSION_BLOCK, FUSION_MAX_BLOCKS, _random_colour
from test_gpu_fusion_weighted import SUM_RTOL, TWIST, _assert_record, _random_model, _random_weights
from test_gpu_rigid3d import _depth
from test_rigid3d_host import K_SYN

pytestmark = pytest.mark.gpu

assert SUM_RTOL == 1e-12
# (Z, Y, X) and a fractional array offset that puts the synthetic surface (z = 250 voxels) through the volume: 315 voxels
# (78 four-voxel steps and a tail of 3, one workgroup) and 32^3 (32 workgroups)
VOLUMES = [((5, 7, 9), np.array([-4.5, -3.25, 247.5])), ((32, 32, 32), np.array([-16.5, -16.25, 234.75]))]
SHIFT = (2, -1, -3)  # x, y, z: three distinct components
DTYPES = [np.uint16, np.float32, np.float64]


@pytest.fixture(scope="module")
def lsf():
    import levelsetfusion_python_amd as m
    return m


def _camera(K_, ratio=0.001):
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    return DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=K_), depth_unit_ratio=ratio)


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _device(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


@functools.lru_cache(maxsize=None)
def _inputs(depth_dtype):
    """the rigid tests' depth image, a random colour image and the pathological weight image; made once, never written"""
    d = _depth(depth_dtype)
    rng = np.random.default_rng(17)
    image = rng.integers(0, 256, d.shape + (3,)).astype(np.uint8)
    pw = _random_weights(d.shape, rng)  # exact 0, negative, NaN, +inf and tiny weights among them
    for a in (d, image, pw):
        a.setflags(write=False)
    return d, image, pw


def _offset_view(a):
    """a device copy of `a` that starts 4 bytes past a 16-byte boundary"""
    big = torch.empty(a.size + 4, dtype=torch.float32, device="cuda")
    view = big[1:a.size + 1].view(a.shape)
    assert view.data_ptr() % 16 == 4
    view.copy_(torch.from_numpy(a))
    return view


def _unpack(rec):
    from levelsetfusion_python_amd.device_fusion import unpack_warped_record
    return unpack_warped_record(rec.cpu().numpy())


def _assert_warped_record(got, want):
    _assert_record(got, want)
    for key in ("coloured", "first_coloured", "warp_rejected"):
        assert got[key] == want[key], (key, got, want)


def _call(t, W, c, warp, d, image, pw, off, carve, band=0.25, unaligned=False, w=0.5, cap=CAP):
    """the device call on fresh copies: (tsdf, weight, colour or None, record tensor); c None: no colour"""
    from levelsetfusion_python_amd import device_fusion
    from levelsetfusion_python_amd.tsdf import generation as gen
    dev, code = gen.device_depth(d)
    a_t, a_w, a_p = (_offset_view(a) for a in (t, W, warp)) if unaligned else _device(t, W, warp)
    a_c, img = (None, None) if c is None else _device(c, image)
    pw_dev = None if pw is None else _device(pw)[0]
    rec = device_fusion.integrate_depth_warped(a_t, a_w, dev, code, _camera(K_SYN), off, TWIST, a_p, w=w, max_weight=cap,
                                               pixel_weight=pw_dev, carve=carve, colour=a_c, colour_image=img,
                                               colour_band=band)
    assert rec.dtype == torch.float64 and rec.is_cuda and rec.shape == (9,)
    return a_t, a_w, a_c, rec


def _unwarped(t, W, c, d, image, pw, off, carve, band=0.25, w=0.5, cap=CAP):
    """the existing entry points on fresh copies: the weighted call, or the colour call when c is given"""
    from levelsetfusion_python_amd import device_fusion
    from levelsetfusion_python_amd.tsdf import generation as gen
    dev, code = gen.device_depth(d)
    a_t, a_w = _device(t, W)
    pw_dev = None if pw is None else _device(pw)[0]
    if c is None:
        rec = device_fusion.integrate_depth_weighted(a_t, a_w, dev, code, _camera(K_SYN), off, TWIST, w=w, max_weight=cap,
                                                     pixel_weight=pw_dev, carve=carve)
        return a_t, a_w, None, rec
    a_c, img = _device(c, image)
    rec = device_fusion.integrate_depth_colour(a_t, a_w, a_c, dev, code, _camera(K_SYN), off, TWIST, img, w=w,
                                               max_weight=cap, pixel_weight=pw_dev, carve=carve, colour_band=band)
    return a_t, a_w, a_c, rec


def _assert_same_as_unwarped(got, want, size):
    for a, b in zip(got[:3], want[:3]):
        assert (a is None) == (b is None)
        assert a is None or _bits_equal(a.cpu().numpy(), b.cpu().numpy())
    g, u = got[3].cpu().numpy(), want[3].cpu().numpy()
    assert np.array_equal(g[:8].view(np.uint64), u.view(np.uint64)) and g[8] == 0
    assert u[0] > (1000 if size > 1000 else 0)


# ------------------------------------------------------------------------------- 1. psi = 0: the existing entry points
@pytest.mark.parametrize("depth_dtype", DTYPES)
def test_a_zero_warp_equals_the_existing_entry_points(lsf, depth_dtype):
    d, image, pw = _inputs(depth_dtype)
    rng = np.random.default_rng(29)
    for shape, off in VOLUMES:
        t, W = _random_model(shape, rng, CAP)
        c = _random_colour(shape, rng)
        zero = np.zeros(shape + (3,), np.float32)
        signs = np.where(rng.integers(0, 2, shape + (3,)) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        for weights, carve, colour in ((None, False, None), (None, True, None), (pw, False, None), (pw, True, c)):
            want = _unwarped(t, W, colour, d, image, weights, off, carve)
            for warp, unaligned in ((zero, False), (signs, True)):
                got = _call(t, W, colour, warp, d, image, weights, off, carve, unaligned=unaligned)
                _assert_same_as_unwarped(got, want, t.size)
            if colour is not None:
                assert want[3].cpu().numpy()[6] > (500 if t.size > 1000 else 0)
        if t.size > 1000:  # without arguments: the unweighted entry point's result
            from levelsetfusion_python_amd import device_fusion
            from levelsetfusion_python_amd.tsdf import generation as gen
            dev, code = gen.device_depth(d)
            u_t, u_w = _device(t, W)
            plain = device_fusion.integrate_depth(u_t, u_w, dev, code, _camera(K_SYN), off, TWIST, w=0.5,
                                                  max_weight=CAP).cpu().numpy()
            got = _call(t, W, None, zero, d, image, None, off, False)
            assert _bits_equal(got[0].cpu().numpy(), u_t.cpu().numpy())
            assert _bits_equal(got[1].cpu().numpy(), u_w.cpu().numpy())
            assert np.array_equal(got[3].cpu().numpy()[:4].view(np.uint64), plain[:4].view(np.uint64))


# ---------------------------------------------------------------------------- 2. a constant integer psi: a shifted offset
@pytest.mark.parametrize("depth_dtype", DTYPES)
def test_a_constant_integer_warp_equals_a_shifted_array_offset(lsf, depth_dtype):
    """channel 0 is x, 1 is y, 2 is z, and a voxel's three floats are its own: (index + psi) + offset and
    index + (offset + psi) are exact in float64 for these values"""
    d, image, pw = _inputs(depth_dtype)
    rng = np.random.default_rng(31)
    for shape, off in VOLUMES:
        t, W = _random_model(shape, rng, CAP)
        c = _random_colour(shape, rng)
        warp = np.broadcast_to(np.array(SHIFT, np.float32), shape + (3,)).copy()
        shifted = off + np.array(SHIFT, np.float64)
        for weights, carve, colour in ((None, False, None), (pw, True, c)):
            want = _unwarped(t, W, colour, d, image, weights, shifted, carve)
            for unaligned in (False, True):
                got = _call(t, W, colour, warp, d, image, weights, off, carve, unaligned=unaligned)
                _assert_same_as_unwarped(got, want, t.size)
        if t.size > 1000:  # and the test tells the channel orders apart
            other = _unwarped(t, W, None, d, image, None, off + np.array(SHIFT[::-1], np.float64), False)
            assert not _bits_equal(other[0].cpu().numpy(), want[0].cpu().numpy())


# ------------------------------------------------------------------------------------- 3. a general psi: the restatement
def _random_warp(shape, rng):
    """psi in [-2, 2]^3 with a few NaN and infinite entries and a few finite ones that leave the image"""
    warp = rng.uniform(-2, 2, shape + (3,)).astype(np.float32)
    flat = warp.reshape(-1)
    flat[7::97] = np.nan
    flat[11::131] = np.inf
    flat[13::151] = -np.inf
    flat[17::173] = 1e5
    flat[19::211] = -3e4
    return warp


@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("carve", [False, True])
def test_a_general_warp_against_the_restatement(lsf, carve, weighted, colour):
    rng = np.random.default_rng(37)
    for (shape, off), depth_dtype, unaligned in zip(VOLUMES + VOLUMES[:1], (np.float32, np.uint16, np.float64),
                                                    (False, False, True)):
        d, image, pw = _inputs(depth_dtype)
        pw = pw if weighted else None
        t, W = _random_model(shape, rng, CAP)
        c = _random_colour(shape, rng) if colour else None
        warp = _random_warp(shape, rng)
        a_t, a_w, a_c, rec = _call(t, W, c, warp, d, image, pw, off, carve, unaligned=unaligned)
        want_t, want_w, want_c, want = WR.fuse_depth_warped(t, W, d, K_SYN, 0.001, off, TWIST, warp, 20, 0.004, 0.5, CAP,
                                                            pw, carve, c, image if colour else None, 0.25)
        assert _bits_equal(a_t.cpu().numpy(), want_t) and _bits_equal(a_w.cpu().numpy(), want_w)
        assert (a_c is None) == (want_c is None) and (a_c is None or _bits_equal(a_c.cpu().numpy(), want_c))
        got = _unpack(rec)
        _assert_warped_record(got, want)
        assert got["warp_rejected"] == np.count_nonzero(~np.isfinite(warp).all(axis=-1)) > 0
        if t.size > 1000:
            assert got["fused"] > 1000 and got["warp_rejected"] > 500
            assert (got["weight_rejected"] > 100) == weighted and (got["carved"] > 500) == carve
            assert (got["coloured"] > 500) == colour and (0 < got["first_coloured"] < got["coloured"]) == colour
            # the field moves what a voxel sees: the zero field's result differs
            zero = WR.fuse_depth_warped(t, W, d, K_SYN, 0.001, off, TWIST, np.zeros_like(warp), 20, 0.004, 0.5, CAP, pw,
                                        carve)[0]
            assert np.count_nonzero(zero != want_t) > 1000


def test_reruns_are_bit_identical(lsf):
    d, image, pw = _inputs(np.uint16)
    shape, off = VOLUMES[1]
    rng = np.random.default_rng(41)
    t, W = _random_model(shape, rng, CAP)
    c = _random_colour(shape, rng)
    warp = _random_warp(shape, rng)
    first = _call(t, W, c, warp, d, image, pw, off, True)
    again = _call(t, W, c, warp, d, image, pw, off, True)
    for x, y in zip(first, again):
        assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))


# ------------------------------------------------------------------------------------ 4. the second trip of the capped grid
def test_second_trip_of_the_capped_grid(lsf):
    groups = int(np.prod(BIG)) // 4
    first_trip = FUSION_BLOCK * FUSION_MAX_BLOCKS
    assert groups > first_trip and int(np.prod((128, 128, 128))) // 4 <= first_trip  # the smallest cube of planes that crosses
    past = 4 * first_trip  # the flat index of the first voxel of the second trip
    d, image, pw = _inputs(np.uint16)
    rng = np.random.default_rng(43)
    t, W = _random_model(BIG, rng, CAP)
    c = _random_colour(BIG, rng)
    warp = _random_warp(BIG, rng)
    want_t, want_w, want_c, want = WR.fuse_depth_warped(t, W, d, K_SYN, 0.001, BIG_OFF, TWIST, warp, 20, 0.004, 0.5, CAP,
                                                        pw, True, c, image, 0.25)
    updated = (want_t.reshape(-1).view(np.uint32) != t.reshape(-1).view(np.uint32))
    coloured = np.any(want_c.reshape(-1, 4).view(np.uint32) != c.reshape(-1, 4).view(np.uint32), axis=1)
    assert np.count_nonzero(updated[past:]) > 1000 and np.count_nonzero(updated[:past]) > 1000
    assert np.count_nonzero(updated[past:past + 4 * FUSION_BLOCK]) > 100  # among the first workgroup's second step
    assert np.count_nonzero(coloured[past:]) > 1000
    assert np.count_nonzero(~np.isfinite(warp).all(axis=-1).reshape(-1)[past:]) > 100
    a_t, a_w, a_c, rec = _call(t, W, c, warp, d, image, pw, BIG_OFF, True)
    assert _bits_equal(a_t.cpu().numpy(), want_t) and _bits_equal(a_w.cpu().numpy(), want_w)
    assert _bits_equal(a_c.cpu().numpy(), want_c)
    _assert_warped_record(_unpack(rec), want)


# ------------------------------------------------------------------------------------------------------ 5. end to end
@functools.lru_cache(maxsize=None)
def _restated_chain():
    """frame 0 fused, the live volume of frame 1, the oracle's warp from the model to it, frame 1 fused through it: (model
    tsdf and weight after frame 0, psi, tsdf, weight and record after frame 1, tsdf after a rigid frame 1)"""
    from oracle import lsf_oracle as O
    d0, d1 = D.frames()
    shape = (D.N,) * 3
    gen = (D.K, 1.0, D.OFFSET, D.TWIST, D.BAND, D.VOXEL)
    t0, W0, _ = FW.fuse_depth_weighted(np.ones(shape, np.float32), np.zeros(shape, np.float32), d0, *gen)
    live = R3.live_volume(d1, D.K, 1.0, shape, D.OFFSET, D.TWIST, D.BAND, D.VOXEL)
    psi = O.HierarchicalOracle(**D.OPTIMIZER).optimize(t0, live)
    assert psi.dtype == np.float32 and psi.shape == shape + (3,) and np.isfinite(psi).all()
    t1, W1, _, rec = WR.fuse_depth_warped(t0, W0, d1, D.K, 1.0, D.OFFSET, D.TWIST, psi, D.BAND, D.VOXEL)
    rigid = FW.fuse_depth_weighted(t0, W0, d1, *gen)[0]
    return t0, W0, psi, t1, W1, rec, rigid


def _sequence(lsf, optimizer=True, **kw):
    opt = lsf.HierarchicalOptimizer3d(**D.OPTIMIZER) if optimizer else None
    return lsf.SequenceFusion3d(_camera(D.K, 1.0), D.N, D.OFFSET, voxel_size=D.VOXEL, narrow_band_width_voxels=D.BAND,
                                rigid_iterations=0, nonrigid_optimizer=opt, **kw)


def test_a_growing_sphere_is_fused_through_the_warp_field(lsf):
    """the condition: fused through psi, frame 1 changes the model near its surface by less than half of what it
    changes it by when fused rigidly (the restated chain gives 0.024 against 0.212); and the model is the restated
    chain's, bit for bit"""
    t0, W0, psi, t1, W1, want, rigid_t1 = _restated_chain()
    d0, d1 = D.frames()
    seq, rigid = _sequence(lsf), _sequence(lsf, optimizer=False)
    first = seq.integrate(d0)
    rigid.integrate(d0)
    assert seq.warp is None and first["nonrigid"] is None and tuple(first["fusion"]) == lsf.fusion.RECORD_FIELDS
    assert _bits_equal(seq.canonical.tsdf.cpu().numpy(), t0) and _bits_equal(seq.canonical.weight.cpu().numpy(), W0)
    frame = seq.integrate(d1)
    rigid.integrate(d1)
    got_t, rigid_t = seq.canonical.tsdf.cpu().numpy(), rigid.canonical.tsdf.cpu().numpy()
    with_warp, without = D.model_change(t0, got_t), D.model_change(t0, rigid_t)
    print("mean |change| near the surface: %.6f through the warp field, %.6f rigidly" % (with_warp, without))
    assert with_warp < 0.5 * without
    assert _bits_equal(rigid_t, rigid_t1)
    assert seq.warp.is_cuda and seq.warp.dtype == torch.float32 and tuple(seq.warp.shape) == (D.N,) * 3 + (3,)
    assert _bits_equal(seq.warp.cpu().numpy(), psi)
    assert _bits_equal(got_t, t1) and _bits_equal(seq.canonical.weight.cpu().numpy(), W1)
    assert tuple(frame["fusion"]) == lsf.fusion.WARPED_RECORD_FIELDS
    _assert_warped_record(frame["fusion"], want)
    assert frame["fusion"]["fused"] > 1000 and frame["fusion"]["warp_rejected"] == 0
    assert frame["nonrigid"] is seq.nonrigid_optimizer.engine.last_call and frame["nonrigid"] is not None
    assert np.array_equal(frame["twist"], np.zeros(6)) and len(seq.frame_records) == 2


def test_a_growing_sphere_with_carving_and_colour(lsf):
    d0, d1 = D.frames()
    image = D.colour_image()
    plain, seq = _sequence(lsf, carve=True), _sequence(lsf, carve=True, colour=True)
    for d in (d0, d1):
        a, b = plain.integrate(d), seq.integrate(d, image)
        assert b["fusion"]["coloured"] > 1000 and b["fusion"]["carved"] > 1000
        assert {k: b["fusion"][k] for k in a["fusion"] if k not in ("coloured", "first_coloured")} \
            == {k: v for k, v in a["fusion"].items() if k not in ("coloured", "first_coloured")}
    assert tuple(b["fusion"]) == tuple(a["fusion"]) == lsf.fusion.WARPED_RECORD_FIELDS and a["fusion"]["coloured"] == 0
    assert b["fusion"]["first_coloured"] < b["fusion"]["coloured"]  # frame 1 averages into frame 0's colours
    assert _bits_equal(seq.warp.cpu().numpy(), plain.warp.cpu().numpy())
    assert _bits_equal(seq.canonical.tsdf.cpu().numpy(), plain.canonical.tsdf.cpu().numpy())
    assert _bits_equal(seq.canonical.weight.cpu().numpy(), plain.canonical.weight.cpu().numpy())
    # on an empty model carving changes weights alone, so the model after frame 0 and the warp are the uncarved run's
    assert _bits_equal(seq.warp.cpu().numpy(), _restated_chain()[2])
    verts, faces, colours = seq.extract_mesh(colours=True)
    assert len(verts) > 1000 and len(faces) > 1000 and colours.dtype == np.uint8
    assert np.array_equal(colours, np.broadcast_to(np.array(D.COLOUR, np.uint8), (len(verts), 3)))
    plain_verts, plain_faces = plain.extract_mesh()
    assert _bits_equal(verts, plain_verts) and np.array_equal(faces, plain_faces)


def test_the_volume_takes_a_warp(lsf):
    """CanonicalVolume.integrate_depth(..., warp=): numpy or device, with and without a colour image"""
    d, image, pw = _inputs(np.float32)
    shape, off = VOLUMES[1]
    rng = np.random.default_rng(47)
    t, W = _random_model(shape, rng, CAP)
    c = _random_colour(shape, rng)
    warp = _random_warp(shape, rng)
    cam = _camera(K_SYN)
    for colour in (False, True):
        want_t, want_w, want_c, want = WR.fuse_depth_warped(t, W, d, K_SYN, 0.001, off, TWIST, warp, 20, 0.004, 0.5, CAP,
                                                            pw, True, c if colour else None, image if colour else None,
                                                            0.25)
        for field in (warp, _device(warp)[0]):
            vol = lsf.fusion.CanonicalVolume(shape, max_weight=CAP, colour=True)
            vol.tsdf.copy_(torch.from_numpy(t)), vol.weight.copy_(torch.from_numpy(W))
            vol.colour.copy_(torch.from_numpy(c))
            rec = vol.integrate_depth(d, cam, TWIST, off, weight=0.5, pixel_weight=pw, carve=True,
                                      colour_image=image if colour else None, colour_band=0.25, warp=field)
            assert _bits_equal(vol.tsdf.cpu().numpy(), want_t) and _bits_equal(vol.weight.cpu().numpy(), want_w)
            assert _bits_equal(vol.colour.cpu().numpy(), want_c if colour else c)
            _assert_warped_record(lsf.fusion.unpack_warped_record(rec.cpu().numpy()), want)
    with pytest.raises(ValueError, match="float32"):
        vol.integrate_depth(d, cam, TWIST, off, warp=warp.astype(np.float64))
    with pytest.raises(ValueError, match="colour=True"):
        lsf.fusion.CanonicalVolume(shape).integrate_depth(d, cam, TWIST, off, colour_image=image, warp=warp)


def test_host_refuses_bad_arguments(lsf):
    from levelsetfusion_python_amd import device_fusion
    from levelsetfusion_python_amd.tsdf import generation as gen
    d, image, _ = _inputs(np.uint16)
    dev, code = gen.device_depth(d)
    cam = _camera(K_SYN)
    t, w = torch.ones((8, 8, 8), device="cuda"), torch.zeros((8, 8, 8), device="cuda")
    c = torch.zeros((8, 8, 8, 4), device="cuda")
    psi = torch.zeros((8, 8, 8, 3), device="cuda")
    img, = _device(image)
    args = (dev, code, cam, [0, 0, 0], np.zeros(6))
    with pytest.raises(TypeError, match="torch tensor"):
        device_fusion.integrate_depth_warped(t, w, *args, psi.cpu().numpy())
    with pytest.raises(ValueError, match="one device"):
        device_fusion.integrate_depth_warped(t, w, *args, psi.cpu())
    with pytest.raises(ValueError, match="float32"):
        device_fusion.integrate_depth_warped(t, w, *args, psi.double())
    with pytest.raises(ValueError, match=r"\+ \(3,\)"):
        device_fusion.integrate_depth_warped(t, w, *args, psi[..., :2].contiguous())
    with pytest.raises(ValueError, match="contiguous"):
        device_fusion.integrate_depth_warped(t, w, *args, torch.zeros((3, 8, 8, 8), device="cuda").permute(1, 2, 3, 0))
    both = torch.zeros(8 * 8 * 8 * 4, device="cuda")
    with pytest.raises(ValueError, match="alias tsdf"):
        device_fusion.integrate_depth_warped(both[:512].view(8, 8, 8), w, *args, both[:1536].view(8, 8, 8, 3))
    with pytest.raises(ValueError, match="alias colour"):
        device_fusion.integrate_depth_warped(t, w, *args, both[:1536].view(8, 8, 8, 3), colour=both.view(8, 8, 8, 4),
                                             colour_image=img)
    for kw in (dict(colour=c), dict(colour_image=img)):
        with pytest.raises(ValueError, match="together"):
            device_fusion.integrate_depth_warped(t, w, *args, psi, **kw)
    with pytest.raises(ValueError, match="colour_band"):
        device_fusion.integrate_depth_warped(t, w, *args, psi, colour=c, colour_image=img, colour_band=1.5)
    with pytest.raises(ValueError, match="one shape"):
        device_fusion.integrate_depth_warped(t, w, *args, psi, pixel_weight=torch.ones((3, 3), device="cuda"))
    assert torch.all(t == 1) and torch.all(w == 0) and not c.any()  # nothing was launched
