"""CPU checks of colour fusion ("Colour fusion"): the numpy restatement
(tests/colour_restatement.py) against hand-computed voxels, the coloured PLY round trip, the two new symbols of the built
library, the argument errors that are raised before a GPU is asked for, and the painted scene (tests/colour_scene.py)
whose margins the GPU test relies on."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import colour_restatement as C
import colour_scene as CS
import fusion_scene as S

F32 = np.float32


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------- the restatement, voxel by voxel
IMAGE = np.array([[[10, 20, 30], [200, 100, 50]], [[255, 0, 7], [1, 2, 3]]], np.uint8)  # (2, 2, 3)


def _one(l, colour, pixel=(0, 1), valid=True, **kw):
    """colour_update of a single voxel that projects to `pixel`"""
    got, counts = C.colour_update(np.array([colour], F32), np.array([l], F32), np.array([pixel[0]]),
                                  np.array([pixel[1]]), np.array([valid]), IMAGE, **kw)
    return got[0], counts


def test_a_first_colour_is_the_pixel_s_and_an_average_follows_the_rule():
    got, counts = _one(0.1, [0, 0, 0, 0], w=1.0)
    assert _bits_equal(got, [200, 100, 50, 1]) and counts == {"coloured": 1, "first_coloured": 1}
    # Wc = 3, C = (30, 60, 90), w = 0.5 at pixel (200, 100, 50): each channel (3 C + 0.5 c) / 3.5 in float32
    got, counts = _one(-0.2, [30, 60, 90, 3], w=0.5)
    want = [(F32(3) * F32(c0) + F32(0.5) * F32(c1)) / F32(3.5) for c0, c1 in ((30, 200), (60, 100), (90, 50))]
    assert _bits_equal(got, want + [F32(3.5)]) and counts == {"coloured": 1, "first_coloured": 0}
    assert _bits_equal(want, [F32(190) / F32(3.5), F32(230) / F32(3.5), F32(295) / F32(3.5)])


@pytest.mark.parametrize("band", [1.0, 0.25])
def test_band_edges_are_strict(band):
    old = [30, 60, 90, 3]
    inside = np.nextafter(F32(band), F32(0))
    for l, coloured in ((band, False), (-band, False), (inside, True), (-inside, True), (np.nan, False)):
        got, counts = _one(l, old, colour_band=band)
        assert counts["coloured"] == int(coloured), l
        assert _bits_equal(got, old) != coloured
    if band < 1:  # a voxel that the geometry rule fuses (in band) and the colour rule leaves alone
        got, counts = _one(0.5, old, colour_band=band)
        assert _bits_equal(got, old) and counts == {"coloured": 0, "first_coloured": 0}


def test_a_carved_voxel_is_never_coloured():
    """l == 1 with a valid pixel: fused as +1 by the geometry rule under carve, outside every colour band"""
    for band in (1.0, 0.25):
        got, counts = _one(1.0, [30, 60, 90, 3], colour_band=band)
        assert _bits_equal(got, [30, 60, 90, 3]) and counts == {"coloured": 0, "first_coloured": 0}
    got, counts = _one(0.1, [30, 60, 90, 3], valid=False)  # and so is a voxel without a valid pixel
    assert _bits_equal(got, [30, 60, 90, 3]) and counts["coloured"] == 0


def test_a_rejected_weight_leaves_the_colour_alone():
    for bad in (0.0, -0.5, np.nan, np.inf):
        pw = np.ones((2, 2), F32)
        pw[0, 1] = bad
        got, counts = _one(0.1, [30, 60, 90, 3], pixel_weight=pw)
        assert _bits_equal(got, [30, 60, 90, 3]) and counts == {"coloured": 0, "first_coloured": 0}, bad
    pw = np.full((2, 2), 0.25, F32)  # a usable one scales w: w_eff = 2 * 0.25
    got, counts = _one(0.1, [30, 60, 90, 3], w=2.0, pixel_weight=pw)
    want = [(F32(3) * F32(c0) + F32(0.5) * F32(c1)) / F32(3.5) for c0, c1 in ((30, 200), (60, 100), (90, 50))]
    assert _bits_equal(got, want + [F32(3.5)]) and counts["coloured"] == 1


def test_the_weight_cap_limits_wc_and_not_the_average():
    got, _ = _one(0.0, [30, 60, 90, 8], w=1.0, max_weight=8.0)
    want = [(F32(8) * F32(c0) + F32(c1)) / F32(9) for c0, c1 in ((30, 200), (60, 100), (90, 50))]
    assert _bits_equal(got, want + [F32(8)])
    got, _ = _one(0.0, [0, 0, 0, 0], w=3.0, max_weight=2.0)
    assert _bits_equal(got, [200, 100, 50, 2])


def test_the_restated_call_keeps_the_weighted_geometry_and_counts_rejections_once():
    import fusion_weighted_restatement as FW
    rng = np.random.default_rng(3)
    shape, off = (24, 24, 24), S.offset(24)
    depth, image, _ = CS.frames()[1]
    t = rng.uniform(-1, 1, shape).astype(F32)
    w = rng.choice(np.array([0, 1, 2.5], F32), shape)
    c = np.zeros(shape + (4,), F32)
    pw = rng.uniform(0.1, 2, depth.shape).astype(F32)
    pw[::3, ::2] = 0
    args = (depth, S.K, 1.0, off, S.true_twist(1), 20, 0.004, 0.5, 4.0, pw, True)
    got_t, got_w, got_c, rec = C.fuse_depth_colour(t, w, c, depth, image, *args[1:], colour_band=0.25)
    want_t, want_w, want = FW.fuse_depth_weighted(t, w, *args)
    assert _bits_equal(got_t, want_t) and _bits_equal(got_w, want_w)
    assert {k: rec[k] for k in want} == want and want["weight_rejected"] > 0 and want["carved"] > 0
    assert 0 < rec["coloured"] < rec["fused"] and rec["first_coloured"] == rec["coloured"]
    changed = np.any(got_c != 0, axis=-1)
    assert np.count_nonzero(changed) == rec["coloured"] and not np.any(changed & (got_w == w))


def test_colour_bytes_round_half_up_and_clamp():
    got = C.colour_byte([-3.0, 0.49, 0.5, 1.5, 254.5, 255.0, 300.0, np.nan, np.inf, -np.inf])
    assert got.dtype == np.uint8 and got.tolist() == [0, 0, 1, 2, 255, 255, 255, 0, 255, 0]


def test_restated_vertex_colours_follow_the_table():
    """one crossing x edge, a = -0.25 at voxel v and b = 0.75 at w, so t = 0.25"""
    t = np.ones((2, 2, 2), F32)
    t[0, 0, 0], t[0, 0, 1] = -0.25, 0.75
    w = np.ones_like(t)
    import mesh_restatement as M
    verts, _, _ = M.extract(t, w, [0, 0, 0], 1.0)
    assert len(verts) == 3 and np.array_equal(verts[0], [0.25, 0, 0])  # the x edge's vertex comes first
    for wa, wb, want in ((1, 2, [10 * 0.75 + 110 * 0.25, 20 * 0.75 + 120 * 0.25, 255]), (1, 0, [10, 20, 255]),
                         (0, 2, [110, 120, 0]), (0, 0, [1, 2, 3]), (np.nan, 2, [110, 120, 0])):
        c = np.zeros((2, 2, 2, 4), F32)
        c[0, 0, 0], c[0, 0, 1] = [10, 20, 300, wa], [110, 120, -4, wb]
        got = C.vertex_colours(t, w, c, default_colour=(1, 2, 3))
        assert got.shape == (3, 3) and got.dtype == np.uint8
        if wa == 1 and wb == 2:
            want = [int(np.floor(want[0] + 0.5)), int(np.floor(want[1] + 0.5)), 224]  # 300 * 0.75 - 4 * 0.25 = 224
        assert got[0].tolist() == want, (wa, wb)


# ------------------------------------------------------------------------------------------------------------- PLY
def _mesh():
    rng = np.random.default_rng(5)
    verts = rng.normal(size=(7, 3)).astype(F32)
    faces = rng.integers(0, 7, (5, 3)).astype(np.int32)
    normals = rng.normal(size=(7, 3)).astype(F32)
    colours = rng.integers(0, 256, (7, 3)).astype(np.uint8)
    return verts, faces, normals, colours


@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("with_colours", [False, True])
def test_ply_round_trip_with_colours(tmp_path, with_normals, with_colours):
    from levelsetfusion_python_amd import mesh_io
    verts, faces, normals, colours = _mesh()
    path = str(tmp_path / "mesh.ply")
    mesh_io.write_ply(path, verts, faces, normals if with_normals else None, colours=colours if with_colours else None)
    head = open(path, "rb").read().split(b"end_header\n")[0].decode("ascii").split("\n")[:-1]
    floats = 6 if with_normals else 3
    assert head[3:3 + floats] == ["property float %s" % n for n in ("x", "y", "z", "nx", "ny", "nz")[:floats]]
    assert (head[3 + floats:6 + floats] == ["property uchar red", "property uchar green", "property uchar blue"]) \
        == with_colours
    v, f, n, c = mesh_io.read_ply(path, colours=True)
    assert _bits_equal(v, verts) and np.array_equal(f, faces) and f.dtype == np.int32
    assert (n is None) != with_normals and (c is None) != with_colours
    assert n is None or _bits_equal(n, normals)
    assert c is None or (c.dtype == np.uint8 and np.array_equal(c, colours))
    if with_colours:  # the three-tuple reader refuses a coloured file as it always has
        with pytest.raises(ValueError, match="unexpected PLY layout after the vertex properties"):
            mesh_io.read_ply(path)
    else:
        out = mesh_io.read_ply(path)
        assert len(out) == 3 and _bits_equal(out[0], verts) and np.array_equal(out[1], faces)


def test_ply_colour_errors(tmp_path):
    from levelsetfusion_python_amd import mesh_io
    verts, faces, normals, colours = _mesh()
    path = str(tmp_path / "bad.ply")
    with pytest.raises(ValueError, match="rows"):
        mesh_io.write_ply(path, verts, faces, colours=colours[:-1])
    with pytest.raises(ValueError, match="uint8"):
        mesh_io.write_ply(path, verts, faces, colours=colours.astype(np.float32))
    with pytest.raises(ValueError, match="uint8"):
        mesh_io.write_ply(path, verts, faces, colours=colours.astype(np.int32))
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        mesh_io.write_ply(path, verts, faces, colours=np.zeros((7, 4), np.uint8))
    empty = np.zeros((0, 3), F32), np.zeros((0, 3), np.int32)
    mesh_io.write_ply(path, *empty, colours=np.zeros((0, 3), np.uint8))
    v, f, n, c = mesh_io.read_ply(path, colours=True)
    assert v.shape == (0, 3) and f.shape == (0, 3) and n is None and c.shape == (0, 3) and c.dtype == np.uint8


# ------------------------------------------------------------------------------------------- the library and the host
def test_the_built_library_exports_the_two_entry_points():
    import levelsetfusion_python_amd as lsf
    L = lsf._lib
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in ("lsf_fusion_integrate_depth_colour", "lsf_mesh_vertex_colours"):
        assert hasattr(raw, name) and name in L.PROTOTYPES and getattr(L.lib, name).restype is ctypes.c_int
    assert L.FUSION_COLOUR_SCRATCH_BYTES == L.FUSION_MAX_BLOCKS * 8 * 8
    assert L.FusionColourParams.colour_band.offset == ctypes.sizeof(L.FusionWeightedParams)
    assert ctypes.sizeof(L.FusionColourParams) == ctypes.sizeof(L.FusionWeightedParams) + 8
    # the host refuses before anything touches a device
    p = L.FusionColourParams()
    assert L.lib.lsf_fusion_integrate_depth_colour(None, None, None, None, None, None, None, None, ctypes.byref(p),
                                                   None) == -1
    assert L.lib.lsf_mesh_vertex_colours(None, None, None, None, None, 1, 0, 0, 256, ctypes.byref(L.MeshParams()),
                                         None) == -1


# a child without torch and with every GPU hidden: the entry point's own refusals are host code, and a call that a
# refusal should have stopped must find no device to launch on
_CHILD = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
count = ctypes.c_int(-1)
hidden = lib.hipGetDeviceCount(ctypes.byref(count)) != 0 or count.value == 0
fn = lib.lsf_fusion_integrate_depth_colour
fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p] * 10
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
    """lsf_fusion_integrate_depth_colour's refusals behind the wrapper's: a misaligned colour buffer, each overlap of
    the pairwise matrix at the last byte of the earlier buffer (the colour volume's extent is four times the model's),
    colour_band outside (0, 1].  Made-up addresses: every case must return before a launch"""
    import torch
    import levelsetfusion_python_amd as lsf
    from levelsetfusion_python_amd import device_fusion, device_rigid
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    L = lsf._lib
    cam = DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=S.K), depth_unit_ratio=0.001)
    shape, (h, w) = (8, 8, 8), (6, 8)
    model, pixels = 8 * 8 * 8 * 4, h * w
    sizes = dict(tsdf=model, weight=model, colour=4 * model, depth=2 * pixels, pixel_weight=4 * pixels, image=3 * pixels)
    names = ("tsdf", "weight", "colour", "depth", "pixel_weight", "image", "record", "scratch")
    base = {name: 0x10000000 + 0x100000 * i for i, name in enumerate(names)}

    def params(band=1.0, has_pixel_weight=1):
        p = L.FusionColourParams()
        p.weighted.fusion = device_fusion._params(shape, 1.0, np.inf)
        p.weighted.fusion.tsdf = device_rigid._tsdf3d(np.asarray(S.K), cam, torch.zeros((h, w), dtype=torch.int16),
                                                      0.004, 20., 1)
        p.weighted.fusion.depth_dtype = L.DEPTH_U16
        p.weighted.carve, p.weighted.has_pixel_weight, p.colour_band = 1, has_pixel_weight, band
        return bytes(p).hex()

    def case(passes=False, params_=None, **moved):
        at = dict(base, **moved)
        return dict(passes=passes, params=params_ or params(), pointers=[at[name] for name in names])

    refused = {"colour not 16-byte aligned": case(colour=base["colour"] + 4),
               "no colour volume": case(colour=None), "no colour image": case(image=None),
               "pixel_weight without has_pixel_weight": case(params_=params(has_pixel_weight=0)),
               "has_pixel_weight without pixel_weight": case(pixel_weight=None)}
    for band in (0.0, -0.25, 1.5, float("nan"), float("inf")):
        refused["colour_band %r" % band] = case(params_=params(band=band))
    order = ("tsdf", "weight", "colour", "depth", "pixel_weight", "image")
    for i, first in enumerate(order):  # the later buffer begins on the earlier one's last byte (or last record)
        for second in order[i + 1:]:
            step = 16 if second == "colour" else 1
            refused["%s overlaps %s" % (second, first)] = case(**{second: base[first] + sizes[first] - step})
            refused["%s overlaps %s" % (first, second)] = case(**{second: base[first] - sizes[second] + step})
    passing = {"the plain call": case(passes=True),
               "no pixel_weight": case(passes=True, params_=params(has_pixel_weight=0), pixel_weight=None),
               "colour_band 0.25": case(passes=True, params_=params(band=0.25)),
               "image right behind colour": case(passes=True, image=base["colour"] + sizes["colour"]),
               "image right before colour": case(passes=True, image=base["colour"] - sizes["image"])}
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


def test_argument_errors_come_before_the_gpu():
    import levelsetfusion_python_amd as lsf
    from levelsetfusion_python_amd import device_fusion, device_mesh
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    cam = DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=S.K), depth_unit_ratio=1.0)
    with pytest.raises(ValueError, match="nonrigid_optimizer"):
        lsf.SequenceFusion3d(cam, 32, S.offset(32), nonrigid_optimizer=object(), colour=True)
    for bad in (0.0, -0.25, 1.5, np.nan, np.inf):
        with pytest.raises(ValueError, match="colour_band"):
            lsf.SequenceFusion3d(cam, 32, S.offset(32), colour=True, colour_band=bad)
        with pytest.raises(ValueError, match="colour_band"):
            device_fusion.colour_band_of(bad)
    assert device_fusion.colour_band_of(1.0) == 1.0 and device_fusion.colour_band_of(0.25) == 0.25
    with pytest.raises(ValueError, match="3-D"):
        lsf.fusion.CanonicalVolume((16, 16), colour=True)
    for bad in ((1, 2), (0, 0, 256), (-1, 0, 0), (0.5, 1, 2)):
        with pytest.raises(ValueError, match="default_colour"):
            device_mesh.default_colour_of(bad)
    assert device_mesh.default_colour_of((0, 128, 255)) == (0, 128, 255)
    rec = lsf.fusion.unpack_colour_record(np.array([5, 2, 1.5, 0.75, 7, 3, 4, 1], np.float64))
    assert rec == {"fused": 5, "first_seen": 2, "sum_abs_change": 1.5, "max_abs_change": 0.75, "carved": 7,
                   "weight_rejected": 3, "coloured": 4, "first_coloured": 1}
    assert lsf.fusion.COLOUR_RECORD_FIELDS == lsf.fusion.WEIGHTED_RECORD_FIELDS + ("coloured", "first_coloured")
    assert tuple(rec) == lsf.fusion.COLOUR_RECORD_FIELDS


# ------------------------------------------------------------------------------------------------------- the scene
def test_the_painted_scene_is_fusion_scene_s():
    for k, (depth, image, surface) in enumerate(CS.frames()):
        assert _bits_equal(depth, S.render(S.true_twist(k)))
        assert image.dtype == np.uint8 and image.shape == depth.shape + (3,)
        assert np.array_equal(surface >= 0, depth > 0) and set(np.unique(surface)) == {0, 1, 2, 3}
        assert np.array_equal(image[surface == 2], np.broadcast_to(CS.COLOURS[2], (np.count_nonzero(surface == 2), 3)))


def test_the_restated_scene_meets_its_margins():
    """the condition of the GPU scene test, on the restatement alone: the margins exclude at most 20 % of the vertices,
    and every vertex they keep has exactly its surface's colour"""
    _, _, c, records, (verts, faces, _, colours) = CS.restated_model()
    assert len(verts) > 3000 and len(colours) == len(verts)
    assert all(r["coloured"] > 1000 for r in records) and records[0]["first_coloured"] == records[0]["coloured"]
    assert all(0 < r["coloured"] < r["fused"] for r in records)  # the colour band is a part of the band
    ok, sid = CS.qualifying(verts)
    assert np.count_nonzero(~ok) <= CS.EXCLUDED_CAP * len(verts), (np.count_nonzero(~ok), len(verts))
    assert np.array_equal(colours[ok], CS.COLOURS[sid[ok]])
    kept = np.bincount(sid[ok], minlength=4)
    assert np.count_nonzero(kept >= 100) >= 2, kept  # more than one surface is held to its colour
