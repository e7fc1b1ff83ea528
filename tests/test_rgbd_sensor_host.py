"""Host checks of the RGB-D sensor front end (no GPU): properties of the numpy restatement (tests/rgbd_restatement.py)
that the HIP kernels are then held to bit for bit -- the identity, no gaps on a plane under scaling, translation, barrel
distortion and rotation, occlusion by the z-buffer --, the rig scene (tests/rgbd_rig_scene.py) registered, rectified and
fused by the existing restatements with every qualifying mesh vertex carrying its surface's colour exactly, and the host
rules of fusion.RgbdSensor: coefficient padding, the three sources of depth_to_colour, the ValueErrors and
from_infinitam_format."""
import io
import os

import numpy as np
import pytest

import colour_scene as CS
import rgbd_restatement as G
import rgbd_rig_scene as RS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

PLANE_SHAPE = (48, 64)
PLANE_K = np.array([[60.0, 0, 31.5], [0, 60.0, 23.5], [0, 0, 1]])
WIDE_K, WIDE_SHAPE = np.array([[100.0, 0, 51.5], [0, 100.0, 39.5], [0, 0, 1]]), (80, 104)
TWICE_K, TWICE_SHAPE = np.array([[120.0, 0, 63.5], [0, 120.0, 47.5], [0, 0, 1]]), (96, 128)


@pytest.fixture(scope="module")
def lsf():
    import levelsetfusion_python_amd as m
    return m


def plane_cases():
    """name -> (depth, lens coefficients, depth_to_output, K_out, out_shape): the constant planes of the contract"""
    one = np.full(PLANE_SHAPE, 1.0, np.float32)
    return {
        "twice the focal length": (one, None, np.eye(4), TWICE_K, TWICE_SHAPE),
        "translated into a wider camera": (one, None, G.transform(t=(0.05, 0, 0)), WIDE_K, WIDE_SHAPE),
        "barrel into the same camera": (np.full(PLANE_SHAPE, 0.75, np.float32), G.BARREL, np.eye(4), PLANE_K,
                                        PLANE_SHAPE),
        "barrel, rotated and translated": (one, G.BARREL, G.transform((0, 0.03, 0), (0.03, 0.005, 0)), WIDE_K,
                                           WIDE_SHAPE),
    }


def occlusion_case():
    """a wall at 1.0 with a 16 x 16 patch at 0.5, seen from 5 cm to the side through the same camera"""
    depth = np.full(PLANE_SHAPE, 1.0, np.float32)
    depth[12:28, 20:36] = 0.5
    return depth, None, G.transform(t=(0.05, 0, 0)), PLANE_K, PLANE_SHAPE


def behind_case():
    """the near half of the image lies behind an output camera that stands 0.2 m further along the axis"""
    depth = np.full(PLANE_SHAPE, 1.0, np.float32)
    depth[:, :32] = 0.1
    return depth, None, G.transform(t=(0, 0, -0.2)), PLANE_K, PLANE_SHAPE


def registered(depth, k, T, K_out, out_shape, K=PLANE_K, ratio=1.0, **kw):
    corner, centre = G.ray_table(*depth.shape, K, k)
    return G.register_depth(depth, ratio, corner, centre, T, K_out, out_shape, **kw)


def filled_box(filled):
    rows, cols = np.nonzero(filled.any(axis=1))[0], np.nonzero(filled.any(axis=0))[0]
    return slice(rows[0], rows[-1] + 1), slice(cols[0], cols[-1] + 1)


def enclosed_holes(filled):
    """the empty pixels with filled pixels on both sides in their row and in their column"""
    def between(axis):
        before = np.maximum.accumulate(filled, axis=axis)
        after = np.flip(np.maximum.accumulate(np.flip(filled, axis), axis=axis), axis)
        return before & after
    return ~filled & between(0) & between(1)


def test_undistortion_inverts_the_lens_and_leaves_a_pinhole_exact():
    corner, centre = G.ray_table(7, 9, PLANE_K, None)
    u, v = np.arange(9.0), np.arange(7.0)
    assert np.array_equal(centre[..., 0], np.broadcast_to((u - 31.5) / 60.0, (7, 9)))
    assert np.array_equal(corner[..., 1], np.broadcast_to((((np.arange(8.0) - 0.5) - 23.5) / 60.0)[:, None], (8, 10)))
    for k in (G.BARREL, RS.COLOUR_COEFFS, (-0.2, 0.05, 0.001, -0.0005, 0.01, 0.02, -0.01, 0.003)):
        _, centre = G.ray_table(*PLANE_SHAPE, PLANE_K, k)
        xd, yd = G.distort(centre[..., 0], centre[..., 1], k)
        vv, uu = np.meshgrid(np.arange(48.0), np.arange(64.0), indexing="ij")
        assert np.abs(60.0 * xd + 31.5 - uu).max() < 1e-4 and np.abs(60.0 * yd + 23.5 - vv).max() < 1e-4
    # the iteration count matters: five steps leave more than eight do, on the contract's lens and field
    x, y = np.meshgrid(np.linspace(-0.45, 0.45, 31), np.linspace(-0.35, 0.35, 23))
    xd, yd = G.distort(x, y, G.BARREL)
    miss = [np.abs(np.stack(G.undistort(xd, yd, G.BARREL, n)) - np.stack([x, y])).max() for n in (5, 8, 10)]
    assert miss[0] > miss[1] > miss[2] and miss[1] < 1e-7 and miss[0] < 1e-4


def test_identity_returns_the_depth_bit_for_bit():
    rng = np.random.default_rng(5)
    depth = rng.uniform(0.3, 4.0, PLANE_SHAPE).astype(np.float32)
    depth[rng.random(PLANE_SHAPE) < 0.1] = 0.0
    out, rec = registered(depth, None, np.eye(4), PLANE_K, PLANE_SHAPE)
    assert np.array_equal(out.view(np.uint32), depth.view(np.uint32))
    n = int(np.count_nonzero(depth))
    assert rec == dict(valid=n, behind=0, outside=0, empty=0, clipped=0, written=n, filled=n, masked=0)


def test_no_gaps_on_a_plane():
    cases = plane_cases()
    out, rec = registered(*cases["twice the focal length"])
    assert np.all(out == 1.0) and rec["clipped"] == 0 and rec["filled"] == out.size
    out, rec = registered(*cases["translated into a wider camera"])
    box = filled_box(out != 0)
    assert np.all(out[box] == 1.0) and out[box].size == rec["filled"] > 0.5 * out.size and rec["clipped"] == 0
    out, rec = registered(*cases["barrel into the same camera"])
    assert np.all(out == np.float32(0.75)) and rec["clipped"] == 0
    out, rec = registered(*cases["barrel, rotated and translated"])
    assert rec["filled"] > 0.5 * out.size and rec["clipped"] == 0
    assert not enclosed_holes(out != 0).any()


def test_the_nearer_surface_wins_and_what_it_uncovers_stays_empty():
    out, rec = registered(*occlusion_case())
    # the patch moves 60 * 0.05 / 0.5 = 6 pixels, the wall 3
    assert np.all(out[12:28, 26:42] == 0.5)
    assert np.all(out[12:28, 23:26] == 0.0)  # the three columns the patch uncovers: nothing is seen there
    expect = np.full(PLANE_SHAPE, 1.0, np.float32)
    expect[:, :3] = 0.0  # no depth pixel lands left of the wall's first
    expect[12:28, 23:26] = 0.0
    expect[12:28, 26:42] = 0.5
    assert np.array_equal(out, expect)
    assert rec["valid"] == 48 * 64 and rec["outside"] > 0  # the wall's last columns leave the image
    assert rec["written"] + rec["outside"] == rec["valid"] and rec["behind"] == rec["empty"] == rec["clipped"] == 0


def test_records_count_every_fate_of_a_pixel():
    rng = np.random.default_rng(6)
    # ranges that hold no pixel, and some that share one: a fine image into a coarse one
    depth = rng.uniform(0.5, 2.0, (96, 128)).astype(np.float32)
    K = np.array([[120.0, 0, 63.5], [0, 120.0, 47.5], [0, 0, 1]])
    K_out = np.array([[30.0, 0, 15.5], [0, 30.0, 11.5], [0, 0, 1]])
    out, rec = registered(depth, None, np.eye(4), K_out, (24, 32), K=K)
    assert rec["empty"] > 0 and rec["written"] > rec["filled"] > 0.9 * 24 * 32 and rec["valid"] == depth.size
    assert rec["valid"] == rec["behind"] + rec["outside"] + rec["empty"] + rec["written"]
    # a coarse image into a fine one: the footprint is cut to max_footprint from the low end
    depth = np.full((5, 6), 1.0, np.float32)
    K = np.array([[6.0, 0, 2.5], [0, 6.0, 2.0], [0, 0, 1]])
    K_out = np.array([[96.0, 0, 47.5], [0, 96.0, 39.5], [0, 0, 1]])
    out, rec = registered(depth, None, np.eye(4), K_out, (80, 96), K=K, max_footprint=4)
    assert rec["clipped"] == 30 and rec["filled"] == 30 * 16
    assert np.all(out[0:4, 0:4] == 1.0) and np.all(out[4:16, 0:16][:, 4:] == 0.0)
    # part of the image behind the output camera
    out, rec = registered(*behind_case())
    assert rec["behind"] == 48 * 32 and rec["written"] > 0 and rec["clipped"] == 0
    assert rec["valid"] == rec["behind"] + rec["outside"] + rec["empty"] + rec["written"]
    # a mask takes filled pixels away and counts them
    depth = np.full(PLANE_SHAPE, 1.0, np.float32)
    valid = (rng.random(PLANE_SHAPE) < 0.7).astype(np.uint8)
    out, rec = registered(depth, None, np.eye(4), PLANE_K, PLANE_SHAPE, colour_valid=valid)
    assert rec["masked"] == int((valid == 0).sum()) > 0 and np.array_equal(out != 0, valid != 0)


def test_rectification_resamples_bilinearly_and_marks_what_has_no_source():
    rng = np.random.default_rng(7)
    src = rng.integers(0, 256, (30, 40, 3), dtype=np.uint8)
    K = np.array([[40.0, 0, 19.5], [0, 40.0, 14.5], [0, 0, 1]])
    same, valid = G.rectify_colour(src, K, None, K, (30, 40))
    assert np.array_equal(same, src) and np.all(valid == 1)  # an ideal lens into its own camera: the identity
    dst, valid = G.rectify_colour(src, K, RS.COLOUR_COEFFS, K, (30, 40))
    assert 0 < int(valid.sum()) <= valid.size and np.all(dst[valid == 0] == 0)
    wide = np.array([[25.0, 0, 29.5], [0, 25.0, 19.5], [0, 0, 1]])
    dst, valid = G.rectify_colour(src, K, RS.COLOUR_COEFFS, wide, (40, 60))
    assert np.any(valid == 0) and np.any(valid == 1) and np.all(dst[valid == 0] == 0)
    # a constant image stays constant where it has a source: the weights sum to one
    flat = np.full((30, 40, 3), 200, np.uint8)
    dst, valid = G.rectify_colour(flat, K, RS.COLOUR_COEFFS, wide, (40, 60))
    assert np.all(dst[valid == 1] == 200)


def test_the_rig_scene_fuses_to_exact_colours():
    """the raw pairs of the rig registered and rectified by the restatement, fused by the existing restatements: every
    vertex colour_scene.qualifying accepts carries its surface's colour exactly (4562 vertices, 18.4 % excluded, none
    wrong when this was written)"""
    registration = RS.restated_registration()
    assert len(registration) == CS.FRAMES
    for depth_m, colour, valid, rec in registration:
        assert depth_m.shape == RS.COLOUR_SHAPE and colour.shape == RS.COLOUR_SHAPE + (3,)
        assert rec["clipped"] == 0 and rec["behind"] == 0 and rec["masked"] > 0
        assert rec["filled"] > 0.9 * depth_m.size  # the depth camera sees nearly all of the colour camera's field
        assert rec["valid"] == rec["outside"] + rec["empty"] + rec["written"]
        assert np.all(depth_m[valid == 0] == 0)
    _, _, _, (verts, _, colours) = RS.restated_model()
    ok, sid = CS.qualifying(verts)
    assert len(verts) > 4000 and ok.sum() > 3000
    assert 1.0 - ok.mean() <= CS.EXCLUDED_CAP
    assert np.array_equal(colours[ok], CS.COLOURS[sid[ok]])


# ---- fusion.RgbdSensor's host rules ---------------------------------------------------------------------------------------

def test_coefficients_are_padded_and_checked(lsf):
    from levelsetfusion_python_amd import device_rgbd as D
    assert np.array_equal(D.coefficients(None), np.zeros(8))
    assert np.array_equal(D.coefficients([]), np.zeros(8))
    assert np.array_equal(D.coefficients(G.BARREL), list(G.BARREL) + [0, 0, 0, 0])
    assert np.array_equal(D.coefficients(np.array(RS.COLOUR_COEFFS).reshape(5, 1)), list(RS.COLOUR_COEFFS) + [0, 0, 0])
    assert np.array_equal(D.coefficients(np.arange(8.0).reshape(1, 8)), np.arange(8.0))
    for k in ([1.0], np.zeros(6), np.zeros(9), [0, 0, np.nan, 0], [np.inf] * 8):
        with pytest.raises(ValueError):
            D.coefficients(k)
    for k in (None, G.BARREL, RS.COLOUR_COEFFS):
        assert np.array_equal(D.coefficients(k), G.coefficients(k))
    sensor = lsf.fusion.RgbdSensor(*RS.cameras())
    assert np.array_equal(sensor.depth_coefficients, G.coefficients(G.BARREL))
    assert np.array_equal(sensor.colour_coefficients, G.coefficients(RS.COLOUR_COEFFS))
    # the package's own DepthCamera passes as it is: no coefficients, an ideal lens
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    plain = lsf.fusion.RgbdSensor(DepthCamera(intrinsic_matrix=PLANE_K, depth_unit_ratio=0.001))
    assert not plain.depth_coefficients.any() and plain.depth_unit_ratio == 0.001
    assert np.array_equal(plain.camera.intrinsics.intrinsic_matrix, PLANE_K) and plain.camera.depth_unit_ratio == 1.0
    assert np.array_equal(plain.depth_to_colour, np.eye(4))


def test_the_three_sources_of_depth_to_colour(lsf):
    depth_camera, colour_camera = RS.cameras()
    S = lsf.fusion.RgbdSensor
    assert np.array_equal(S(depth_camera, colour_camera).depth_to_colour, np.eye(4))

    class Extrinsics:
        rotation = RS.DEPTH_TO_COLOUR[:3, :3]
        translation = RS.DEPTH_TO_COLOUR[:3, 3].reshape(1, 3)  # the reference keeps it as a row

    colour_camera.extrinsics = Extrinsics()
    assert np.array_equal(S(depth_camera, colour_camera).depth_to_colour, RS.DEPTH_TO_COLOUR)
    given = G.transform((0.01, 0, 0), (0, 0.02, 0))
    assert np.array_equal(S(depth_camera, colour_camera, given).depth_to_colour, given)
    sensor = S(depth_camera, colour_camera)
    assert np.array_equal(sensor.camera.intrinsics.intrinsic_matrix, RS.COLOUR_K) and not sensor.colour_passes
    assert S(depth_camera, RS.Camera(RS.COLOUR_K)).colour_passes
    assert not S(depth_camera, RS.Camera(RS.COLOUR_K), output_intrinsics=PLANE_K).colour_passes
    other = S(depth_camera, colour_camera, output_intrinsics=WIDE_K)
    assert np.array_equal(other.camera.intrinsics.intrinsic_matrix, WIDE_K)


def test_value_errors(lsf):
    depth_camera, colour_camera = RS.cameras()
    S = lsf.fusion.RgbdSensor
    for bad in (np.eye(3), np.zeros((4, 3)), np.full((4, 4), np.nan), [[1, 0, 0, np.inf]] * 4):
        with pytest.raises(ValueError):
            S(depth_camera, colour_camera, bad)
    with pytest.raises(ValueError):
        S(depth_camera, None, np.eye(4))  # a transform into a colour camera there is none of
    with pytest.raises(ValueError):
        S(RS.Camera(RS.DEPTH_K), colour_camera)  # no depth_unit_ratio
    with pytest.raises(ValueError):
        S(object())
    for f in (0, 17, 2.5):
        with pytest.raises(ValueError):
            S(depth_camera, colour_camera, max_footprint=f)
    with pytest.raises(ValueError):
        S(RS.Camera(np.array([[0.0, 0, 1], [0, 5, 1], [0, 0, 1]]), None, 1.0))  # fx = 0
    with pytest.raises(ValueError):
        S(depth_camera, colour_camera, output_intrinsics=np.array([[1.0, 0, 1], [0, np.nan, 1], [0, 0, 1]]))
    # a colour image without a colour camera
    alone = S(depth_camera)
    with pytest.raises(ValueError, match="colour_camera"):
        alone.admit(RS.DEPTH_SHAPE, RS.COLOUR_SHAPE + (3,))
    with pytest.raises(ValueError, match="colour_camera"):
        alone.register(np.zeros(RS.DEPTH_SHAPE, np.float32), np.zeros(RS.COLOUR_SHAPE + (3,), np.uint8))
    alone.admit(RS.DEPTH_SHAPE)
    assert alone.output_shape == RS.DEPTH_SHAPE
    # an image whose extents differ from the first call's
    with pytest.raises(ValueError, match="first frame"):
        alone.admit((RS.DEPTH_SHAPE[0], RS.DEPTH_SHAPE[1] + 1))
    both = S(depth_camera, colour_camera)
    with pytest.raises(ValueError, match="output_shape"):
        both.admit(RS.DEPTH_SHAPE)  # nothing says how large the output is
    both.admit(RS.DEPTH_SHAPE, RS.COLOUR_SHAPE + (3,))
    assert both.output_shape == RS.COLOUR_SHAPE
    both.admit(RS.DEPTH_SHAPE)  # a frame without colour after one with
    with pytest.raises(ValueError, match="first colour frame"):
        both.admit(RS.DEPTH_SHAPE, (RS.COLOUR_SHAPE[0] + 2, RS.COLOUR_SHAPE[1], 3))
    with pytest.raises(ValueError, match="first frame"):
        both.register(np.zeros((10, 10), np.float32))
    # the sequence's own rules
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    Seq = lsf.fusion.SequenceFusion3d
    with pytest.raises(ValueError, match="sensor.camera"):
        Seq(DepthCamera(intrinsic_matrix=RS.COLOUR_K), 16, np.zeros(3), sensor=both)
    with pytest.raises(ValueError):
        Seq(None, 16, np.zeros(3))
    with pytest.raises(ValueError):
        Seq(None, 16, np.zeros(3), sensor=depth_camera)


INLINE_CALIB = """640 480
504.261 503.905
352.457 272.202

512 424
573.71 574.394
346.471 249.031

0.999749 0.00518867 0.0217975 0.0243073
-0.0051649 0.999986 -0.0011465 -0.000166518
-0.0218031 0.00103363 0.999762 0.0151706

affine 0.0002 0.0
"""


def test_from_infinitam_format(lsf):
    S = lsf.fusion.RgbdSensor
    sensor = S.from_infinitam_format(os.path.join(GOLDEN, "snoopy_calib.txt"))
    K = np.array([[517.0, 0, 320], [0, 517.0, 240], [0, 0, 1]])
    assert np.array_equal(sensor.depth_matrix, K) and np.array_equal(sensor.colour_matrix, K)
    assert np.array_equal(sensor.depth_to_colour, np.eye(4)) and sensor.depth_unit_ratio == 0.001  # a ratio of 0
    assert sensor.output_shape == (480, 640) and sensor.colour_passes
    assert not sensor.depth_coefficients.any() and not sensor.colour_coefficients.any()
    assert np.array_equal(sensor.camera.intrinsics.intrinsic_matrix, K)
    written = np.vstack([np.array([[float(v) for v in line.split()] for line in INLINE_CALIB.splitlines()[8:11]]),
                         [0, 0, 0, 1.0]])
    for source in (io.StringIO(INLINE_CALIB), ):
        sensor = S.from_infinitam_format(source)
        assert np.array_equal(sensor.colour_matrix, [[504.261, 0, 352.457], [0, 503.905, 272.202], [0, 0, 1]])
        assert np.array_equal(sensor.depth_matrix, [[573.71, 0, 346.471], [0, 574.394, 249.031], [0, 0, 1]])
        assert sensor.depth_unit_ratio == 0.0002 and sensor.output_shape == (480, 640)
        # InfiniTAM stores colour-to-depth: the sensor's transform is its inverse
        assert np.allclose(sensor.depth_to_colour @ written, np.eye(4), atol=1e-12)
        assert not np.allclose(sensor.depth_to_colour, written, atol=1e-3)
    as_written = S.from_infinitam_format(io.StringIO(INLINE_CALIB), extrinsic="depth_to_colour", max_footprint=4)
    assert np.array_equal(as_written.depth_to_colour, written) and as_written.max_footprint == 4
    with pytest.raises(ValueError):
        S.from_infinitam_format(io.StringIO(INLINE_CALIB), extrinsic="sideways")
    with pytest.raises(ValueError):
        S.from_infinitam_format(io.StringIO(INLINE_CALIB.replace("0.999749 ", "")))


def test_header_binding_exports_and_documents_agree(lsf):
    header = open(lsf._build.ABI_HEADER).read()
    L = lsf._lib
    for macro, value in (("LSF_RGBD_UNDISTORT_ITERATIONS", L.RGBD_UNDISTORT_ITERATIONS),
                         ("LSF_RGBD_MAX_FOOTPRINT", L.RGBD_MAX_FOOTPRINT),
                         ("LSF_RGBD_DEFAULT_FOOTPRINT", L.RGBD_DEFAULT_FOOTPRINT),
                         ("LSF_RGBD_MAX_BLOCKS", L.RGBD_MAX_BLOCKS), ("LSF_RGBD_RECORD_WORDS", L.RGBD_RECORD_WORDS)):
        assert "#define %s %d\n" % (macro, value) in header, macro
    assert "#define LSF_RGBD_ZBUFFER_EMPTY 0x%xu\n" % L.RGBD_ZBUFFER_EMPTY in header
    assert (G.ITERATIONS, G.MAX_FOOTPRINT, int(G.EMPTY)) == (L.RGBD_UNDISTORT_ITERATIONS, L.RGBD_MAX_FOOTPRINT,
                                                             L.RGBD_ZBUFFER_EMPTY)
    from levelsetfusion_python_amd import device_rgbd as D
    assert D.RECORD_FIELDS == G.RECORD_FIELDS and len(D.RECORD_FIELDS) == L.RGBD_RECORD_WORDS
    assert "lsf_rgbd.hip" in lsf._build.SOURCES
    for name, args in (("lsf_rgbd_ray_table", 4), ("lsf_rgbd_register_depth", 10), ("lsf_rgbd_rectify_colour", 5)):
        assert name + "(" in header and len(L.PROTOTYPES[name][1]) == args
    import ctypes
    assert ctypes.sizeof(L.RgbdParams) == 8 * (4 + 8 + 4 + 9 + 3 + 1) + 4 * 6 and L.RgbdParams.height.offset == 232
    assert "RgbdSensor" in lsf.fusion.__all__ and L.ABI_VERSION == 4
    import inspect
    assert "sensor" in inspect.signature(lsf.fusion.SequenceFusion3d.__init__).parameters
    doc = open(os.path.join(os.path.dirname(lsf._build.ABI_HEADER), "..", "INTEGRATION.md")).read()
    assert "RGB-D sensor" in doc and "lsf_rgbd_register_depth" in doc
    import test_integration_doc as T  # the documented stub still holds, unchanged
    T.test_every_structure_in_the_document_has_the_header_s_member_list()
    T.test_the_stub_checks_the_header_s_abi_identity()


def test_refusals_through_the_c_abi_that_need_no_device(lsf):
    """the host checks run before any launch, so a NULL and a bad parameter are refused without a card"""
    import ctypes
    L = lsf._lib
    from levelsetfusion_python_amd import device_rgbd as D
    p = D.params(shape=(4, 4), K=PLANE_K, out_shape=(4, 4), K_out=PLANE_K)
    assert L.lib.lsf_rgbd_ray_table(None, None, ctypes.byref(p), None) == -1
    assert L.lib.lsf_rgbd_register_depth(None, 1, None, None, None, None, None, None, ctypes.byref(p), None) == -1
    assert L.lib.lsf_rgbd_rectify_colour(None, None, None, ctypes.byref(p), None) == -1
