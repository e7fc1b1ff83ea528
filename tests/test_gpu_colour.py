"""GPU checks of colour fusion and of the mesh's vertex colours (lsf_fusion_integrate_depth_colour in csrc/lsf_fusion.hip,
lsf_mesh_vertex_colours in csrc/lsf_mesh.hip) against the numpy restatement (tests/colour_restatement.py), the existing
entry points and the painted scene (tests/colour_scene.py).  tsdf, weight and the colour volume are compared bit for bit,
the record's counts and maximum exactly, its float64 sum to the 1e-12 relative of tests/fusion_restatement.py, and the
vertex colours as equal uint8."""
import functools

import numpy as np
import pytest
import torch

import colour_restatement as C
import colour_scene as CS
import fusion_scene as S
import mesh_restatement as M
from test_gpu_mesh import _fused, _sphere
from test_gpu_fusion_weighted import SUM_RTOL, TWIST, VOLUMES, _assert_record, _random_model, _random_weights
from test_gpu_rigid3d import _depth
from test_rigid3d_host import K_SYN

pytestmark = pytest.mark.gpu

assert SUM_RTOL == 1e-12
CAP = 6.0
FUSION_BLOCK, FUSION_MAX_BLOCKS = 256, 2048  # kBlock (csrc/lsf_device.h), LSF_FUSION_MAX_BLOCKS (include/lsf_hip.h)
MESH_TILE = 2048  # LSF_MESH_TILE


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


def _random_colour(shape, rng, cap=CAP):
    """a pre-filled colour volume: channels in [0, 255], Wc at 0, between and at the cap"""
    c = rng.uniform(0, 255, shape + (4,)).astype(np.float32)
    c[..., 3] = rng.choice(np.array([0, 0, 1, 2.5, cap], np.float32), shape)
    return c


@functools.lru_cache(maxsize=None)
def _inputs(depth_dtype):
    """the rigid tests' depth image, a random colour image and the pathological weight image; made once, never written"""
    d = _depth(depth_dtype)
    rng = np.random.default_rng(17)
    image = rng.integers(0, 256, d.shape + (3,)).astype(np.uint8)
    pw = _random_weights(d.shape, rng)
    for a in (d, image, pw):
        a.setflags(write=False)
    return d, image, pw


@functools.lru_cache(maxsize=None)
def _seen(depth_dtype, index):
    """what every voxel of VOLUMES[index] sees of the frame under TWIST: shared by the cases that differ in weights,
    carving and band only"""
    shape, off = VOLUMES[index]
    return C.observe(_inputs(depth_dtype)[0], K_SYN, 0.001, shape, off, TWIST)


def _unpack(rec):
    from levelsetfusion_python_amd.device_fusion import unpack_colour_record
    return unpack_colour_record(rec.cpu().numpy())


def _assert_colour_record(got, want):
    _assert_record(got, want)
    for key in ("coloured", "first_coloured"):
        assert got[key] == want[key], (key, got, want)


def _call(t, W, c, d, image, pw, off, carve, band, twist=TWIST, w=0.5, cap=CAP):
    """the device call on fresh copies: (tsdf, weight, colour, record tensor)"""
    from levelsetfusion_python_amd import device_fusion
    from levelsetfusion_python_amd.tsdf import generation as gen
    dev, code = gen.device_depth(d)
    a_t, a_w, a_c, img = _device(t, W, c, image)
    pw_dev = None if pw is None else _device(pw)[0]
    rec = device_fusion.integrate_depth_colour(a_t, a_w, a_c, dev, code, _camera(K_SYN), off, twist, img, w=w,
                                               max_weight=cap, pixel_weight=pw_dev, carve=carve, colour_band=band)
    assert rec.dtype == torch.float64 and rec.is_cuda and rec.shape == (8,)
    return a_t, a_w, a_c, rec


@pytest.mark.parametrize("band", [1.0, 0.25])
@pytest.mark.parametrize("carve", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("depth_dtype", [np.uint16, np.float32, np.float64])
def test_kernel_against_restatement(lsf, depth_dtype, weighted, carve, band):
    d, image, pw = _inputs(depth_dtype)
    pw = pw if weighted else None
    rng = np.random.default_rng(23)
    for index, (shape, off) in enumerate(VOLUMES):
        t, W = _random_model(shape, rng, CAP)
        c = _random_colour(shape, rng)
        a_t, a_w, a_c, rec = _call(t, W, c, d, image, pw, off, carve, band)
        want_t, want_w, want_c, want = C.fuse_depth_colour(t, W, c, d, image, K_SYN, 0.001, off, TWIST, 20, 0.004, 0.5,
                                                           CAP, pw, carve, band, seen=_seen(depth_dtype, index))
        assert _bits_equal(a_t.cpu().numpy(), want_t) and _bits_equal(a_w.cpu().numpy(), want_w)
        assert _bits_equal(a_c.cpu().numpy(), want_c)
        got = _unpack(rec)
        _assert_colour_record(got, want)
        if t.size > 1000:
            assert got["coloured"] > 500 and 0 < got["first_coloured"] < got["coloured"]
            assert (got["coloured"] == got["fused"]) == (band == 1.0)  # the colour band is a part of the band
            assert (got["weight_rejected"] > 100) == weighted and (got["carved"] > 1000) == carve
            at_cap = (c[..., 3] == CAP) & np.any(want_c != c, axis=-1)
            assert np.count_nonzero(at_cap) > 50 and np.all(want_c[at_cap][:, 3] == CAP)  # capped records were averaged


@pytest.mark.parametrize("depth_dtype", [np.uint16, np.float32, np.float64])
def test_geometry_is_the_existing_entry_points(lsf, depth_dtype):
    from levelsetfusion_python_amd import device_fusion
    from levelsetfusion_python_amd.tsdf import generation as gen
    d, image, pw = _inputs(depth_dtype)
    dev, code = gen.device_depth(d)
    cam = _camera(K_SYN)
    rng = np.random.default_rng(29)
    for shape, off in VOLUMES:
        t, W = _random_model(shape, rng, CAP)
        c = _random_colour(shape, rng)
        for weights, carve in ((None, False), (pw, True), (pw, False), (None, True)):
            a_t, a_w, _, rec = _call(t, W, c, d, image, weights, off, carve, 0.25)
            b_t, b_w = _device(t, W)
            want = device_fusion.integrate_depth_weighted(
                b_t, b_w, dev, code, cam, off, TWIST, w=0.5, max_weight=CAP,
                pixel_weight=None if weights is None else _device(weights)[0], carve=carve).cpu().numpy()
            rec = rec.cpu().numpy()
            assert _bits_equal(a_t.cpu().numpy(), b_t.cpu().numpy()) and _bits_equal(a_w.cpu().numpy(), b_w.cpu().numpy())
            assert np.array_equal(rec[:6].view(np.uint64), want[:6].view(np.uint64)) and not want[6:].any()
            if weights is None and not carve:
                u_t, u_w = _device(t, W)
                plain = device_fusion.integrate_depth(u_t, u_w, dev, code, cam, off, TWIST, w=0.5,
                                                      max_weight=CAP).cpu().numpy()
                assert _bits_equal(a_t.cpu().numpy(), u_t.cpu().numpy())
                assert _bits_equal(a_w.cpu().numpy(), u_w.cpu().numpy())
                assert np.array_equal(rec[:6].view(np.uint64), plain[:6].view(np.uint64)) and plain[0] > 0


def test_reruns_are_bit_identical_and_unaligned_models_give_the_aligned_bits(lsf):
    from levelsetfusion_python_amd import device_fusion
    from levelsetfusion_python_amd.tsdf import generation as gen
    d, image, pw = _inputs(np.uint16)
    shape, off = VOLUMES[1]
    rng = np.random.default_rng(31)
    t, W = _random_model(shape, rng, CAP)
    c = _random_colour(shape, rng)
    first = _call(t, W, c, d, image, pw, off, True, 0.25)
    again = _call(t, W, c, d, image, pw, off, True, 0.25)
    for x, y in zip(first, again):
        assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))
    n = t.size
    big = torch.empty(2 * n + 8, dtype=torch.float32, device="cuda")
    tv, wv = big[1:n + 1].view(shape), big[n + 3:2 * n + 3].view(shape)
    assert tv.data_ptr() % 16 and wv.data_ptr() % 16
    tv.copy_(torch.from_numpy(t)), wv.copy_(torch.from_numpy(W))
    dev, code = gen.device_depth(d)
    a_c, img, pw_dev = _device(c, image, pw)
    rec = device_fusion.integrate_depth_colour(tv, wv, a_c, dev, code, _camera(K_SYN), off, TWIST, img, w=0.5,
                                               max_weight=CAP, pixel_weight=pw_dev, carve=True, colour_band=0.25)
    assert _bits_equal(tv.cpu().numpy(), first[0].cpu().numpy()) and _bits_equal(wv.cpu().numpy(), first[1].cpu().numpy())
    assert _bits_equal(a_c.cpu().numpy(), first[2].cpu().numpy())
    assert np.array_equal(rec.cpu().numpy().view(np.uint64), first[3].cpu().numpy().view(np.uint64))


# ------------------------------------------------------------------------------------ the second trip of the capped grid
BIG = (129, 128, 128)
# the synthetic surface (z = 250 voxels, +-16 of tilt, a 15-voxel bump) runs through the last planes: the voxels past the
# cap, planes 128 on, lie inside the band
BIG_OFF = np.array([-64.5, -64.25, 121.75])


def test_second_trip_of_the_capped_grid(lsf):
    groups = int(np.prod(BIG)) // 4
    first_trip = FUSION_BLOCK * FUSION_MAX_BLOCKS
    assert groups > first_trip and int(np.prod((128, 128, 128))) // 4 <= first_trip  # the smallest cube of planes that crosses
    past = 4 * first_trip  # the flat index of the first voxel of the second trip
    d, image, pw = _inputs(np.uint16)
    rng = np.random.default_rng(37)
    t, W = _random_model(BIG, rng, CAP)
    c = _random_colour(BIG, rng)
    want_t, want_w, want_c, want = C.fuse_depth_colour(t, W, c, d, image, K_SYN, 0.001, BIG_OFF, TWIST, 20, 0.004, 0.5, CAP,
                                                       pw, True, 0.25)
    coloured = np.any(want_c.reshape(-1, 4).view(np.uint32) != c.reshape(-1, 4).view(np.uint32), axis=1)
    assert np.count_nonzero(coloured[past:]) > 1000 and np.count_nonzero(coloured[:past]) > 1000
    assert np.count_nonzero(coloured[past:past + 4 * FUSION_BLOCK]) > 20  # among the first workgroup's second step
    a_t, a_w, a_c, rec = _call(t, W, c, d, image, pw, BIG_OFF, True, 0.25)
    assert _bits_equal(a_t.cpu().numpy(), want_t) and _bits_equal(a_w.cpu().numpy(), want_w)
    assert _bits_equal(a_c.cpu().numpy(), want_c)
    _assert_colour_record(_unpack(rec), want)


# ------------------------------------------------------------------------------------------------------- mesh colours
def _noise(shape, seed):
    t = np.random.default_rng(seed).uniform(-1, 1, shape).astype(np.float32)
    t[0] = t[-1] = 1
    t[:, 0] = t[:, -1] = 1
    t[:, :, 0] = t[:, :, -1] = 1
    return t


@functools.lru_cache(maxsize=None)
def _mesh_cases():
    z, y, x = np.meshgrid(*(np.arange(v, dtype=np.float64) for v in (40, 33, 57)), indexing="ij")
    d = np.sqrt(((x - 28.2) / 1.6) ** 2 + (y - 16.1) ** 2 + (z - 19.7) ** 2) - 11.0
    t = np.clip(d / 4, -1, 1).astype(np.float32)
    w = np.random.default_rng(7).uniform(0.0, 3.0, t.shape).astype(np.float32)
    w[w < 0.1] = 0.0
    w[5, 16, :] = np.nan
    t[30, 10:20, 20] = np.nan
    minimal = np.array([[[-0.5, 0.5], [0.25, 0.75]], [[0.1, -0.2], [0.6, 0.3]]], np.float32)
    t[12, 5, 30:40] = np.inf
    sphere = _sphere(24, (11.5, 11.8, 11.3), 8.3)
    fused_t, fused_w, fused_off = _fused(48)  # three frames: weights of 1, 2 and 3, so min_weight 1.5 drops edges
    assert np.any((fused_w > 0) & (fused_w <= 1.5)) and np.any(fused_w > 1.5)
    # (tsdf, weight, array offset, voxel size, iso, min_weight); every volume but the minimal one has more than
    # LSF_MESH_TILE voxels
    return {"noise": (_noise((14, 14, 14), 1), None, [1.5, -2.0, 0.25], 0.01, 0.0, 0.0),
            "non-cubic": (t, w, [-28.0, -16.5, 100.25], 0.004, 0.0, 0.0),
            "iso": (_noise((14, 14, 14), 2), None, [0, 0, 0], 1.0, 0.25, 0.0),
            "sphere": (sphere, None, [0, 0, 0], 1.0, 0.0, 0.0),
            "sphere-iso": (sphere, None, [0, 0, 0], 1.0, 0.25, 0.0),
            "fused-min-weight": (fused_t, fused_w, fused_off, 0.004, 0.0, 1.5),
            "minimal": (minimal, None, [0, 0, 0], 1.0, 0.0, 0.0)}


@pytest.mark.parametrize("name", ["noise", "non-cubic", "iso", "sphere", "sphere-iso", "fused-min-weight",
                                  "minimal"])
def test_mesh_colours_against_restatement(lsf, name):
    t, w, off, voxel, iso, min_weight = _mesh_cases()[name]
    w = np.ones_like(t) if w is None else w
    if name != "minimal":
        assert t.size > MESH_TILE
    rng = np.random.default_rng(41)
    c = rng.uniform(-20, 290, t.shape + (4,)).astype(np.float32)  # channels beyond both ends of a byte
    c[..., 3] = rng.choice(np.array([0, 0, 1, 2.5], np.float32), t.shape)
    c.reshape(-1, 4)[::37, 0] = np.nan
    vol = lsf.fusion.CanonicalVolume(t.shape, colour=True)
    vol.tsdf.copy_(torch.from_numpy(t)), vol.weight.copy_(torch.from_numpy(w)), vol.colour.copy_(torch.from_numpy(c))
    default = (9, 128, 250)
    verts, faces, normals, colours = vol.extract_mesh(off, voxel, iso, min_weight, normals=True, colours=True,
                                                      default_colour=default)
    want = C.vertex_colours(t, w, c, iso, min_weight, default)
    assert colours.dtype == np.uint8 and colours.shape == (len(verts), 3) and np.array_equal(colours, want)
    plain = vol.extract_mesh(off, voxel, iso, min_weight, normals=True)
    assert _bits_equal(verts, plain[0]) and np.array_equal(faces, plain[1]) and _bits_equal(normals, plain[2])
    want_v, want_f, want_n = M.extract(t, w, off, voxel, iso, min_weight, normals=True)
    assert _bits_equal(verts, want_v) and np.array_equal(faces, want_f) and _bits_equal(normals, want_n)
    v2, f2, c2 = vol.extract_mesh(off, voxel, iso, min_weight, colours=True, default_colour=default)
    assert _bits_equal(v2, verts) and np.array_equal(f2, faces) and np.array_equal(c2, colours)
    if name != "minimal":  # every row of the table occurs: both ends, one end either way, neither
        i, j, k, axis = np.nonzero(C._edge_mask(t, w, iso, min_weight))
        wa, wb = c[i, j, k, 3] > 0, c[i + (axis == 2), j + (axis == 1), k + (axis == 0), 3] > 0
        for a in (False, True):
            for b in (False, True):
                assert np.count_nonzero((wa == a) & (wb == b)) > 20
        assert np.count_nonzero(np.all(colours == default, axis=1)) > 20


def test_empty_model_has_no_colours(lsf):
    vol = lsf.fusion.CanonicalVolume((16, 16, 16), colour=True)
    assert vol.colour.shape == (16, 16, 16, 4) and vol.colour.dtype == torch.float32 and not vol.colour.any()
    verts, faces, colours = vol.extract_mesh(S.offset(16), colours=True)
    assert verts.shape == (0, 3) and colours.shape == (0, 3) and colours.dtype == np.uint8
    vol.colour.fill_(3.0)
    vol.reset()
    assert not vol.colour.any() and not vol.weight.any()
    with pytest.raises(ValueError, match="colour=True"):
        lsf.fusion.CanonicalVolume((16, 16, 16)).extract_mesh(S.offset(16), colours=True)


# --------------------------------------------------------------------------------------------------------- the scene
def test_scene_colours(lsf):
    """four painted frames at the true twists, 64^3, colour_band 0.25: the model and its vertex colours equal the
    restatement's, and every vertex clear of the margins has exactly its surface's colour"""
    want_t, want_w, want_c, records, (want_v, want_f, _, want_colours) = CS.restated_model()
    cam = _camera(S.K, 1.0)
    off = CS.offset()
    vol = lsf.fusion.CanonicalVolume(CS.N, colour=True)
    for k, (depth, image, _) in enumerate(CS.frames()):
        rec = vol.integrate_depth(depth, cam, S.true_twist(k), off, colour_image=image, colour_band=CS.COLOUR_BAND)
        _assert_colour_record(_unpack(rec), records[k])
    assert _bits_equal(vol.tsdf.cpu().numpy(), want_t) and _bits_equal(vol.weight.cpu().numpy(), want_w)
    assert _bits_equal(vol.colour.cpu().numpy(), want_c)
    verts, faces, colours = vol.extract_mesh(off, CS.VOXEL, colours=True)
    assert _bits_equal(verts, want_v) and np.array_equal(faces, want_f) and np.array_equal(colours, want_colours)
    ok, sid = CS.qualifying(verts)
    assert np.count_nonzero(~ok) <= CS.EXCLUDED_CAP * len(verts)
    assert np.array_equal(colours[ok], CS.COLOURS[sid[ok]])


# ------------------------------------------------------------------------------------------------------ the sequence
def test_sequence_with_colour(lsf, tmp_path):
    """ "icp" tracking with carving over the painted frames: colour does not change a twist, the records carry the two
    counts of the colour volume, and the model's coloured PLY reads back equal"""
    cam = _camera(S.K, 1.0)
    off = CS.offset()
    kw = dict(tracking_reference="icp", carve=True)
    plain = lsf.SequenceFusion3d(cam, CS.N, off, **kw)
    seq = lsf.SequenceFusion3d(cam, CS.N, off, colour=True, colour_band=CS.COLOUR_BAND, **kw)
    with pytest.raises(ValueError, match="colour_image"):
        seq.integrate(CS.frames()[0][0])
    with pytest.raises(ValueError, match="colour=True"):
        plain.integrate(CS.frames()[0][0], CS.frames()[0][1])
    assert not seq.twists and not plain.twists  # nothing was fused
    for depth, image, _ in CS.frames():
        before = seq.canonical.colour.clone()
        a, b = plain.integrate(depth), seq.integrate(depth, image)
        assert np.array_equal(a["twist"].view(np.uint64), b["twist"].view(np.uint64))
        assert tuple(b["fusion"]) == lsf.fusion.COLOUR_RECORD_FIELDS
        assert {k: b["fusion"][k] for k in a["fusion"]} == a["fusion"] and a["fusion"]["carved"] > 10000
        changed = (seq.canonical.colour != before).any(dim=-1)
        assert b["fusion"]["coloured"] == int(changed.sum()) > 1000  # an average with a new colour changes the weight
        assert b["fusion"]["first_coloured"] == int((changed & (before[..., 3] == 0)).sum())
    assert len(seq.frame_records) == CS.FRAMES and np.any(seq.twists[-1] != 0)
    assert _bits_equal(seq.canonical.tsdf.cpu().numpy(), plain.canonical.tsdf.cpu().numpy())
    verts, faces, normals, colours = seq.extract_mesh(normals=True, colours=True)
    assert len(faces) > 1000 and colours.shape == (len(verts), 3)
    assert np.array_equal(colours, C.vertex_colours(seq.canonical.tsdf.cpu().numpy(), seq.canonical.weight.cpu().numpy(),
                                                    seq.canonical.colour.cpu().numpy()))
    path = str(tmp_path / "model.ply")
    lsf.mesh_io.write_ply(path, verts, faces, normals, colours)
    v, f, n, c = lsf.mesh_io.read_ply(path, colours=True)
    assert _bits_equal(v, verts) and np.array_equal(f, faces) and _bits_equal(n, normals) and np.array_equal(c, colours)


def test_host_refuses_bad_colour_arguments(lsf):
    from levelsetfusion_python_amd import device_fusion
    from levelsetfusion_python_amd.tsdf import generation as gen
    d, image, _ = _inputs(np.uint16)
    dev, code = gen.device_depth(d)
    cam = _camera(K_SYN)
    t, w = torch.ones((8, 8, 8), device="cuda"), torch.zeros((8, 8, 8), device="cuda")
    c = torch.zeros((8, 8, 8, 4), device="cuda")
    img, = _device(image)
    args = (dev, code, cam, [0, 0, 0], np.zeros(6))
    with pytest.raises(ValueError, match=r"\(H, W, 3\)"):
        device_fusion.integrate_depth_colour(t, w, c, *args, img[:-1])
    with pytest.raises(ValueError, match="uint8"):
        device_fusion.integrate_depth_colour(t, w, c, *args, img.float())
    with pytest.raises(ValueError, match="contiguous"):
        device_fusion.integrate_depth_colour(t, w, c, *args, img.transpose(0, 1).contiguous().transpose(0, 1))
    with pytest.raises(TypeError, match="torch tensor"):
        device_fusion.integrate_depth_colour(t, w, c, *args, image)
    with pytest.raises(ValueError, match=r"\+ \(4,\)"):
        device_fusion.integrate_depth_colour(t, w, c[..., :3].contiguous(), *args, img)
    odd = torch.zeros(8 * 8 * 8 * 4 + 1, device="cuda")[1:].view(8, 8, 8, 4)
    assert odd.data_ptr() % 16
    with pytest.raises(ValueError, match="16-byte"):
        device_fusion.integrate_depth_colour(t, w, odd, *args, img)
    both = torch.zeros(8 * 8 * 8 * 5, device="cuda")
    with pytest.raises(ValueError, match="alias"):
        device_fusion.integrate_depth_colour(both[:512].view(8, 8, 8), w, both[:2048].view(8, 8, 8, 4), *args, img)
    for bad in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="colour_band"):
            device_fusion.integrate_depth_colour(t, w, c, *args, img, colour_band=bad)
    with pytest.raises(ValueError, match="colour=True"):
        lsf.fusion.CanonicalVolume(8).integrate_depth(d, cam, np.zeros(6), [0, 0, 0], colour_image=image)
    with pytest.raises(ValueError, match="uint8"):
        lsf.fusion.CanonicalVolume(8, colour=True).integrate_depth(d, cam, np.zeros(6), [0, 0, 0],
                                                                   colour_image=image.astype(np.float32))
    assert torch.all(t == 1) and torch.all(w == 0) and not c.any()  # nothing was launched
