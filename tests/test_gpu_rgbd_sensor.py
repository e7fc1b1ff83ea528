"""GPU checks of the RGB-D sensor front end: lsf_rgbd_ray_table / _register_depth / _rectify_colour (csrc/lsf_rgbd.hip)
against the numpy restatement (tests/rgbd_restatement.py) bit for bit, the records' eight counts included; every
registration run twice with equal bits; the refusals through the C ABI; and the rig scene (tests/rgbd_rig_scene.py)
through fusion.RgbdSensor, CanonicalVolume.integrate_depth and SequenceFusion3d(sensor=).
Sizes: the kernels work a pixel per lane, 256 lanes per workgroup, LSF_RGBD_MAX_BLOCKS workgroups with a stride loop
behind them.  64 x 48 is 12 workgroups; the scene's 512 x 384 and 640 x 480 are 768 and 1200, so their lanes take the
loop's second trip; 9 x 7, 6 x 5 and 1 x 1 are partial workgroups."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import colour_scene as CS
import fusion_scene as S
import rgbd_restatement as G
import rgbd_rig_scene as RS
from test_rgbd_sensor_host import PLANE_K, PLANE_SHAPE, behind_case, occlusion_case, plane_cases

pytestmark = pytest.mark.gpu

GARBAGE = 0x5a5a5a5a  # what outputs and workspaces hold before a call: every word must be written
ALL_EIGHT = (-0.2, 0.05, 0.001, -0.0005, 0.01, 0.02, -0.01, 0.003)


@pytest.fixture(scope="module")
def lsf():
    import levelsetfusion_python_amd as m
    return m


@pytest.fixture(scope="module")
def D(lsf):
    from levelsetfusion_python_amd import device_rgbd
    return device_rgbd


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def _garbage(shape, dtype):
    if dtype == torch.uint8:
        return torch.full(tuple(shape), 0x5a, dtype=torch.uint8, device="cuda")
    if dtype == torch.int64:
        return torch.full(tuple(shape), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device="cuda")
    if dtype == torch.float64:
        return torch.full(tuple(shape), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device="cuda").view(torch.float64)
    t = torch.full(tuple(shape), GARBAGE, dtype=torch.int32, device="cuda")
    return t if dtype == torch.int32 else t.view(torch.float32)


def _bits(t):
    a = t.cpu().numpy()
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8, 2: np.uint16}[a.dtype.itemsize])


def _same_bits(device, host):
    return np.array_equal(_bits(device), np.ascontiguousarray(host).view(_bits(device).dtype))


@pytest.mark.parametrize("k", [None, G.BARREL, ALL_EIGHT], ids=["pinhole", "barrel", "all eight"])
def test_ray_table(D, k):
    K = np.array([[11.0, 0, 4.25], [0, 10.5, 2.75], [0, 0, 1]])
    corner, centre = D.ray_table((7, 9), K, k, _garbage((8, 10, 2), torch.float64), _garbage((7, 9, 2), torch.float64))
    want_corner, want_centre = G.ray_table(7, 9, K, k)
    assert _same_bits(corner, want_corner) and _same_bits(centre, want_centre)
    if k is None:  # the exact pinhole: one subtraction and one division
        assert np.array_equal(centre.cpu().numpy()[..., 0], np.broadcast_to((np.arange(9.0) - 4.25) / 11.0, (7, 9)))


def _register_both(D, depth, k, T, K_out, out_shape, K=PLANE_K, ratio=1.0, max_footprint=8, colour_valid=None):
    """the restated and, twice, the device registration of one case; returns the restated pair after asserting that
    every device word and count equals it and that the two device runs agree bit for bit"""
    want_corner, want_centre = G.ray_table(*depth.shape, K, k)
    want, want_rec = G.register_depth(depth, ratio, want_corner, want_centre, T, K_out, out_shape, max_footprint,
                                      colour_valid)
    corner, centre = D.ray_table(depth.shape, K, k)
    assert _same_bits(corner, want_corner) and _same_bits(centre, want_centre)
    runs = []
    for _ in range(2):
        out, rec = D.register_depth(_dev(depth), corner, centre, T, K_out, out_shape, ratio, max_footprint,
                                    None if colour_valid is None else _dev(colour_valid),
                                    _garbage(out_shape, torch.int32), _garbage(out_shape, torch.float32),
                                    _garbage((8,), torch.int64))
        runs.append((_bits(out), D.unpack_record(rec.cpu().numpy())))
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    assert runs[0][1] == want_rec, (runs[0][1], want_rec)
    assert np.array_equal(runs[0][0], want.view(np.uint32))
    return want, want_rec


@pytest.mark.parametrize("dtype, ratio", [(np.uint16, 0.001), (np.float32, 1.0), (np.float64, 1.0),
                                          (np.float32, 0.001)], ids=["uint16", "float32", "float64", "float32 mm"])
def test_register_depth_types_and_validity(D, dtype, ratio):
    rng = np.random.default_rng(11)
    metres = rng.uniform(0.3, 4.0, PLANE_SHAPE)
    depth = (metres / ratio).astype(dtype)
    depth[rng.random(PLANE_SHAPE) < 0.1] = 0
    if dtype != np.uint16:
        depth[3, 5], depth[7, 11], depth[20, 30], depth[21, 30] = np.nan, np.inf, -1.0, -np.inf
    want, rec = _register_both(D, depth, None, np.eye(4), PLANE_K, PLANE_SHAPE, ratio=ratio)
    live = np.isfinite(depth.astype(np.float64)) & (depth > 0)
    assert rec["valid"] == rec["written"] == rec["filled"] == int(live.sum()) and np.array_equal(want != 0, live)
    if ratio == 1.0:  # the identity: the input's own bits
        assert np.array_equal(want[live].view(np.uint32), depth[live].astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("name", sorted(plane_cases()))
def test_register_planes(D, name):
    want, rec = _register_both(D, *plane_cases()[name])
    assert rec["filled"] > 0 and rec["clipped"] == 0


def test_register_occlusion(D):
    want, _ = _register_both(D, *occlusion_case())
    assert np.all(want[12:28, 26:42] == 0.5) and np.all(want[12:28, 23:26] == 0)


def test_register_fine_into_coarse(D):
    depth = np.random.default_rng(6).uniform(0.5, 2.0, (96, 128)).astype(np.float32)
    K = np.array([[120.0, 0, 63.5], [0, 120.0, 47.5], [0, 0, 1]])
    K_out = np.array([[30.0, 0, 15.5], [0, 30.0, 11.5], [0, 0, 1]])
    _, rec = _register_both(D, depth, None, np.eye(4), K_out, (24, 32), K=K)
    assert rec["empty"] > 0 and rec["written"] > rec["filled"]
    # parallax piles pixels of many depths on the same addresses: the minimum must win whatever the order
    _, rec = _register_both(D, depth, G.BARREL, G.transform((0, 0.05, 0), (0.2, 0.01, 0)), K_out, (24, 32), K=K)
    assert rec["written"] > rec["filled"] > 0
    depth = np.random.default_rng(6).uniform(0.5, 2.0, PLANE_SHAPE).astype(np.float32)
    _, rec = _register_both(D, depth, None, G.transform(t=(0.3, 0, 0)), PLANE_K, PLANE_SHAPE)
    assert rec["written"] > 1.4 * rec["filled"]  # pixels moved 9 to 36 columns by their depth: many on one address


def test_register_clips_a_wide_footprint(D):
    depth = np.full((5, 6), 1.0, np.float32)
    K = np.array([[6.0, 0, 2.5], [0, 6.0, 2.0], [0, 0, 1]])
    K_out = np.array([[96.0, 0, 47.5], [0, 96.0, 39.5], [0, 0, 1]])
    _, rec = _register_both(D, depth, None, np.eye(4), K_out, (80, 96), K=K, max_footprint=4)
    assert rec["clipped"] == 30
    _, rec = _register_both(D, depth, None, np.eye(4), K_out, (80, 96), K=K, max_footprint=16)
    assert rec["clipped"] == 0 and rec["filled"] == 80 * 96


def test_register_behind_one_pixel_and_mask(D):
    _, rec = _register_both(D, *behind_case())
    assert rec["behind"] > 0 and rec["written"] > 0
    depth = np.full(PLANE_SHAPE, 1.0, np.float32)
    want, rec = _register_both(D, depth, None, np.eye(4), np.array([[60.0, 0, -10.0], [0, 60.0, -3.0], [0, 0, 1]]), (1, 1))
    assert rec["filled"] == 1 and rec["outside"] > 0 and want[0, 0] == 1.0
    valid = (np.random.default_rng(8).random(PLANE_SHAPE) < 0.7).astype(np.uint8)
    want, rec = _register_both(D, depth, G.BARREL, np.eye(4), PLANE_K, PLANE_SHAPE, colour_valid=valid)
    assert rec["masked"] == int((valid == 0).sum()) > 0 and np.array_equal(want != 0, valid != 0)


def test_rectify_colour(D):
    src = np.random.default_rng(7).integers(0, 256, (30, 40, 3), dtype=np.uint8)
    K = np.array([[40.0, 0, 19.5], [0, 40.0, 14.5], [0, 0, 1]])
    wide = np.array([[25.0, 0, 29.5], [0, 25.0, 19.5], [0, 0, 1]])
    for K_out, shape in ((K, (30, 40)), (wide, (40, 60))):
        want, want_valid = G.rectify_colour(src, K, RS.COLOUR_COEFFS, K_out, shape)
        dst, valid = D.rectify_colour(_dev(src), K, RS.COLOUR_COEFFS, K_out, shape,
                                      _garbage(shape + (3,), torch.uint8), _garbage(shape, torch.uint8))
        assert np.array_equal(valid.cpu().numpy(), want_valid) and np.array_equal(dst.cpu().numpy(), want)
    assert np.any(want_valid == 0) and np.any(want_valid == 1)


def test_the_shortcut_returns_the_very_tensor(lsf):
    depth_camera = RS.Camera(PLANE_K, None, 1.0)
    sensor = lsf.fusion.RgbdSensor(depth_camera, RS.Camera(PLANE_K))
    image = _dev(np.random.default_rng(9).integers(0, 256, PLANE_SHAPE + (3,), dtype=np.uint8))
    depth = np.full(PLANE_SHAPE, 1.5, np.float32)
    depth_m, colour, rec = sensor.register(depth, image, record=True)
    assert colour is image and sensor.last_colour_valid is None and rec["masked"] == 0
    assert np.array_equal(depth_m.cpu().numpy(), depth) and sensor.ray_residual_px <= 1e-12
    # a lens on the colour camera: rectified, with its validity taken out of the depth
    lens = lsf.fusion.RgbdSensor(depth_camera, RS.Camera(PLANE_K, RS.COLOUR_COEFFS))
    depth_m, colour = lens.register(depth, image)
    want, want_valid = G.rectify_colour(image.cpu().numpy(), PLANE_K, RS.COLOUR_COEFFS, PLANE_K, PLANE_SHAPE)
    assert colour is not image and np.array_equal(colour.cpu().numpy(), want)
    assert np.array_equal(lens.last_colour_valid.cpu().numpy(), want_valid)
    assert np.array_equal(depth_m.cpu().numpy() != 0, want_valid != 0)


def test_a_lens_the_iteration_diverges_on_is_refused(lsf):
    wild = lsf.fusion.RgbdSensor(RS.Camera(PLANE_K, (-4.0, 0, 0, 0), 1.0))
    with pytest.raises(ValueError, match="ray_tolerance_px"):
        wild.register(np.full(PLANE_SHAPE, 1.0, np.float32))
    fine = lsf.fusion.RgbdSensor(RS.Camera(PLANE_K, G.BARREL, 1.0))
    fine.register(np.full(PLANE_SHAPE, 1.0, np.float32))
    assert 0 < fine.ray_residual_px <= 1e-3


def test_refusals_through_the_c_abi(lsf, D):
    L, lib = lsf._lib, lsf._lib.lib
    h, w, ho, wo = 6, 8, 5, 7
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    corner, centre = f64(h + 1, w + 1, 2), f64(h, w, 2)
    depth = torch.ones((h, w), dtype=torch.float32, device="cuda")
    zbuffer = torch.zeros((ho, wo), dtype=torch.int32, device="cuda")
    valid = torch.ones((ho, wo), dtype=torch.uint8, device="cuda")
    out = torch.zeros((ho, wo), dtype=torch.float32, device="cuda")
    record = torch.zeros(8, dtype=torch.int64, device="cuda")
    src = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    dst = torch.zeros((ho, wo, 3), dtype=torch.uint8, device="cuda")

    def good():
        return D.params(shape=(h, w), K=PLANE_K, k=G.BARREL, out_shape=(ho, wo), K_out=PLANE_K)

    def table(p, c=corner, m=centre):
        return lib.lsf_rgbd_ray_table(None if c is None else ptr(c), None if m is None else ptr(m), ctypes.byref(p), None)

    def register(p, d=depth, code=L.DEPTH_F32, c=corner, m=centre, z=zbuffer, v=valid, o=out, r=record):
        args = [None if t is None else ptr(t) for t in (d, c, m, z, v, o, r)]
        return lib.lsf_rgbd_register_depth(args[0], code, *args[1:], ctypes.byref(p), None)

    def rectify(p, s=src, d=dst, v=valid):
        return lib.lsf_rgbd_rectify_colour(*(None if t is None else ptr(t) for t in (s, d, v)), ctypes.byref(p), None)

    assert table(good()) == 0 and register(good()) == 0 and rectify(good()) == 0
    assert register(good(), v=None) == 0  # colour_valid alone may be NULL
    BAD, DIMS = -1, -2
    # a NULL pointer
    assert table(good(), c=None) == table(good(), m=None) == BAD
    for name in "dcmzor":
        assert register(good(), **{name: None}) == BAD, name
    assert rectify(good(), s=None) == rectify(good(), d=None) == rectify(good(), v=None) == BAD
    assert lib.lsf_rgbd_ray_table(ptr(corner), ptr(centre), None, None) == BAD
    assert register(good(), code=3) == BAD
    # an extent below 1
    for field in ("height", "width", "out_height", "out_width"):
        p = good()
        setattr(p, field, 0)
        assert register(p) == BAD and rectify(p) == BAD, field
        if not field.startswith("out"):
            assert table(p) == BAD
    # fx or fy zero or not finite
    for field in ("fx", "fy"):
        for value in (0.0, np.nan, np.inf):
            p = good()
            setattr(p, field, value)
            assert table(p) == BAD and rectify(p) == BAD, (field, value)
            p = good()
            setattr(p, "out_" + field, value)
            assert register(p) == BAD and rectify(p) == BAD, (field, value)
    # a non-finite coefficient, R or t
    for j in range(8):
        p = good()
        p.k[j] = np.nan
        assert table(p) == BAD and rectify(p) == BAD
    for j in range(9):
        p = good()
        p.rotation[j] = np.inf
        assert register(p) == BAD
    for j in range(3):
        p = good()
        p.translation[j] = np.nan
        assert register(p) == BAD
    for value in (0.0, -1.0, np.nan):
        p = good()
        p.depth_unit_ratio = value
        assert register(p) == BAD
    # max_footprint out of range
    for value in (0, -1, L.RGBD_MAX_FOOTPRINT + 1):
        p = good()
        p.max_footprint = value
        assert register(p) == BAD
    # a float64 table that is not 8-byte aligned
    bytes_ = torch.zeros(16 * (h + 1) * (w + 1) + 8, dtype=torch.uint8, device="cuda")
    odd = ctypes.c_void_p(bytes_.data_ptr() + 4)
    assert lib.lsf_rgbd_ray_table(odd, ptr(centre), ctypes.byref(good()), None) == BAD
    assert lib.lsf_rgbd_ray_table(ptr(corner), odd, ctypes.byref(good()), None) == BAD
    assert lib.lsf_rgbd_register_depth(ptr(depth), L.DEPTH_F32, odd, ptr(centre), ptr(zbuffer), None, ptr(out),
                                       ptr(record), ctypes.byref(good()), None) == BAD
    # overlap among inputs, workspaces and outputs
    assert table(good(), c=corner, m=corner) == BAD
    assert register(good(), z=out.view(torch.int32)) == BAD
    assert register(good(), o=depth) == BAD  # 6 x 8 floats cover 5 x 7
    assert register(good(), c=corner, m=corner.view(-1)[:h * w * 2].view(h, w, 2)) == BAD
    big = torch.zeros(4 * ho * wo, dtype=torch.uint8, device="cuda")
    assert rectify(good(), d=big, v=big[ho * wo // 2:]) == BAD
    assert rectify(good(), s=src, d=src) == BAD
    # more pixels than int32 indices reach
    p = good()
    p.height, p.width = 65536, 65536
    assert table(p) == DIMS and register(p) in (BAD, DIMS)
    p = good()
    p.out_height, p.out_width = 65536, 65536
    assert register(p) == DIMS and rectify(p) == DIMS
    torch.cuda.synchronize()
    # the wrapper refuses the same before a launch
    with pytest.raises(ValueError):
        D.register_depth(depth, corner, centre, np.eye(4), PLANE_K, (ho, wo), out_depth=depth)
    with pytest.raises(ValueError):
        D.register_depth(depth, corner, centre[:-1], np.eye(4), PLANE_K, (ho, wo))
    with pytest.raises(ValueError):
        D.register_depth(depth, corner, centre, np.eye(3), PLANE_K, (ho, wo))
    with pytest.raises(ValueError):
        D.rectify_colour(src, PLANE_K, [0.1, np.nan, 0, 0], PLANE_K, (ho, wo))


# ---- the rig scene -----------------------------------------------------------------------------------------------------------

def _sensor(lsf):
    depth_camera, colour_camera = RS.cameras()
    return lsf.fusion.RgbdSensor(depth_camera, colour_camera, RS.DEPTH_TO_COLOUR, max_footprint=RS.MAX_FOOTPRINT)


@functools.lru_cache(maxsize=None)
def _device_registration():
    """FRAMES x (depth_m, colour) device tensors, and the records, of the raw pairs through fusion.RgbdSensor"""
    import levelsetfusion_python_amd as lsf
    sensor = _sensor(lsf)
    out = [sensor.register(depth.copy(), image.copy(), record=True) for depth, image in RS.raw_frames()]
    return sensor, out


def test_the_sensor_registers_the_rig_as_restated(lsf):
    sensor, out = _device_registration()
    assert sensor.output_shape == RS.COLOUR_SHAPE and 0 < sensor.ray_residual_px <= 1e-3
    assert np.array_equal(sensor.camera.intrinsics.intrinsic_matrix, RS.COLOUR_K) and sensor.camera.depth_unit_ratio == 1.0
    for (depth_m, colour, rec), (want, want_colour, _, want_rec) in zip(out, RS.restated_registration()):
        assert rec == want_rec
        assert np.array_equal(_bits(depth_m), want.view(np.uint32))
        assert np.array_equal(colour.cpu().numpy(), want_colour)


def test_the_registered_frames_fuse_to_the_restated_model(lsf):
    sensor, out = _device_registration()
    vol = lsf.fusion.CanonicalVolume(CS.N, colour=True)
    for k, (depth_m, colour, _) in enumerate(out):
        vol.integrate_depth(depth_m, sensor.camera, S.true_twist(k), CS.offset(), colour_image=colour,
                            colour_band=CS.COLOUR_BAND)
    t, w, c, _ = RS.restated_model()
    assert np.array_equal(_bits(vol.tsdf), t.view(np.uint32))
    assert np.array_equal(_bits(vol.weight), w.view(np.uint32))
    assert np.array_equal(_bits(vol.colour), c.view(np.uint32))


def test_a_sequence_with_a_sensor_equals_one_fed_the_registered_pairs(lsf):
    sensor, out = _device_registration()
    settings = dict(colour=True, colour_band=CS.COLOUR_BAND, tracking_reference="icp")
    raw = lsf.fusion.SequenceFusion3d(None, CS.N, CS.offset(), sensor=_sensor(lsf), **settings)
    assert raw.camera is raw.sensor.camera
    registered = lsf.fusion.SequenceFusion3d(sensor.camera, CS.N, CS.offset(), **settings)
    for (depth, image), (depth_m, colour, rec) in zip(RS.raw_frames(), out):
        a = raw.integrate(depth.copy(), image.copy())
        b = registered.integrate(depth_m, colour)
        assert a["registration"] == rec and "registration" not in b
        assert np.array_equal(a["twist"], b["twist"]) and a["fusion"]["fused"] == b["fusion"]["fused"]
    for name in ("tsdf", "weight", "colour"):
        assert np.array_equal(_bits(getattr(raw.canonical, name)), _bits(getattr(registered.canonical, name))), name
    assert np.any(raw.twists[-1] != 0) and len(raw.frame_records[-1]["rigid_records"]) > 0  # the tracker ran
    # colour=False: the sensor gets no colour image, the depth is still registered into the colour camera
    plain = lsf.fusion.SequenceFusion3d(None, CS.N, CS.offset(), tracking_reference="icp",
                                        sensor=lsf.fusion.RgbdSensor(*RS.cameras(), RS.DEPTH_TO_COLOUR,
                                                                     output_shape=RS.COLOUR_SHAPE))
    frame = plain.integrate(RS.raw_frames()[0][0].copy())
    want = dict(RS.restated_registration()[0][3])
    assert frame["registration"]["written"] == want["written"] and frame["registration"]["masked"] == 0
    assert frame["registration"]["filled"] == want["filled"]
    with pytest.raises(ValueError):
        plain.integrate(*RS.raw_frames()[0])
