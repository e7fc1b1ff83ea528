"""CPU checks of the Euclidean distance field: the numpy restatement (tests/esdf_restatement.py) against scipy's exact
transform, its tie rule, its inclusive cap, unknown="occupied", the degenerate models and its accuracy on the sphere
scene against the analytic distance; the header's struct and macros against the binding, the exports, the refusals of
the C entry point in a child with every GPU hidden, and the Python refusals, which all come before a device is asked
for."""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import esdf_cases as C
import esdf_restatement as E
from conftest import ROOT

FAR = E.INT32_MAX


@pytest.fixture(scope="module")
def sphere():
    """the sphere model's transform at R = 64, larger than the 48^3 volume, computed once"""
    tsdf, weight = C.sphere_model()
    distance2, nearest, esdf, record = E.transform(tsdf, weight, C.VOXEL, 64)
    return dict(tsdf=tsdf, weight=weight, distance2=distance2, nearest=nearest, esdf=esdf, record=record)


def _scipy_distance2(site):
    from scipy.ndimage import distance_transform_edt
    return np.rint(distance_transform_edt(~site) ** 2)


def test_restatement_equals_scipy_on_the_sphere_model(sphere):
    site = E.sites(sphere["tsdf"], sphere["weight"])
    assert sphere["record"]["sites"] == int(site.sum()) == 7236
    assert sphere["record"]["finite"] == site.size and not np.any(sphere["distance2"] == FAR)
    assert np.array_equal(sphere["distance2"], _scipy_distance2(site))
    assert sphere["record"]["max_distance2"] == int(sphere["distance2"].max())
    # nearest names a site at exactly that distance
    z, y, x = np.unravel_index(sphere["nearest"], site.shape)
    assert site[z, y, x].all()
    vz, vy, vx = np.indices(site.shape)
    assert np.array_equal((vz - z) ** 2 + (vy - y) ** 2 + (vx - x) ** 2, sphere["distance2"])


def test_restatement_equals_scipy_on_a_random_model():
    tsdf, weight = C.random_model((12, 14, 19), 1)
    site = E.sites(tsdf, weight)
    assert 0 < site.sum() < site.size
    distance2, nearest, esdf, record = E.transform(tsdf, weight, C.VOXEL, 64)
    assert np.array_equal(distance2, _scipy_distance2(site))
    assert np.array_equal(nearest.ravel()[site.ravel()], np.flatnonzero(site))  # a site is its own nearest
    assert distance2.dtype == np.int32 and nearest.dtype == np.int32 and esdf.dtype == np.float32
    assert record == {"sites": int(site.sum()), "finite": site.size, "max_distance2": int(distance2.max())}
    # the box form evaluates the same voxels
    box = ((3, 9), (0, 14), (5, 6))
    part = tuple(slice(a, b) for a, b in box)
    boxed = E.transform(tsdf, weight, C.VOXEL, 3, box=box)
    whole = E.transform(tsdf, weight, C.VOXEL, 3)
    assert boxed[3] is None and all(np.array_equal(b, w[part]) for b, w in zip(boxed[:3], whole[:3]))


def test_sites_are_both_sides_of_a_crossing_between_observed_voxels():
    tsdf = np.array([[[-1, 1, 1, -1, -1, 1, np.nan, -1]]], np.float32)
    weight = np.array([[[1, 1, 1, 1, 0, 1, 1, np.nan]]], np.float32)
    # 0|1 cross; 2|3 cross; 4 and 7 are not observed, so 3|4 and 6|7 make nothing; a NaN tsdf is observed and outside
    assert E.sites(tsdf, weight).ravel().tolist() == [True, True, True, True, False, False, False, False]
    assert E.sites(tsdf, weight, unknown="occupied").ravel().tolist() == [True, True, True, True, True, False, False,
                                                                          True]
    assert E.inside(tsdf, weight).ravel().tolist() == [True, False, False, True, False, False, False, False]
    with pytest.raises(ValueError):
        E.sites(tsdf, weight, unknown="solid")


@pytest.mark.parametrize("name", list(C.TIES))
def test_a_tie_goes_to_the_smallest_flat_index(name):
    shape, pairs, voxel, distance2, tied = C.TIES[name]
    d2, nearest, _, record = E.transform(*C.with_pairs(shape, pairs), C.VOXEL, 6)
    assert record["sites"] == 2 * len(pairs)
    for s in tied:  # the premise: they are sites and equally far
        assert d2[s] == 0 and sum((a - b) ** 2 for a, b in zip(s, voxel)) == distance2
    assert d2[voxel] == distance2
    assert nearest[voxel] == min(C.flat(shape, *s) for s in tied)


def test_the_cap_is_inclusive_and_euclidean():
    tsdf, weight = C.with_pairs(C.CAP_SHAPE, C.CAP_PAIRS)
    d2, nearest, esdf, record = E.transform(tsdf, weight, C.VOXEL, C.CAP_R)
    for voxel, want in C.CAP_EXPECTED.items():
        if want is None:  # R^2 + 1 and beyond, although each offset of the site is <= R
            assert d2[voxel] == FAR and nearest[voxel] == -1, voxel
            assert esdf[voxel] == np.float32(C.CAP_R) * np.float32(C.VOXEL), voxel
        else:
            assert d2[voxel] == want and nearest[voxel] == C.flat(C.CAP_SHAPE, voxel[0], 0, 0), voxel
            assert esdf[voxel] == np.sqrt(np.float32(want)) * np.float32(C.VOXEL), voxel
    assert record["max_distance2"] == C.CAP_R ** 2 and record["finite"] == int((d2 != FAR).sum()) < d2.size
    assert esdf[0, 0, 0] == 0 and np.signbit(esdf[0, 0, 0]) and not np.signbit(esdf[1, 0, 0])  # the inside site: -0.0


def test_unknown_occupied_makes_every_unobserved_voxel_a_site():
    tsdf, weight = C.one_unobserved()
    d2, nearest, esdf, record = E.transform(tsdf, weight, C.VOXEL, 3, unknown="occupied")
    assert record["sites"] == 1 and d2[1, 1, 1] == 0 and nearest[1, 1, 1] == C.flat((4, 4, 4), 1, 1, 1)
    for v in ((0, 1, 1), (2, 1, 1), (1, 0, 1), (1, 2, 1), (1, 1, 0), (1, 1, 2)):  # observed, free, next to unknown
        assert d2[v] == 1 and esdf[v] == np.float32(C.VOXEL)
    assert E.transform(tsdf, weight, C.VOXEL, 3)[3]["sites"] == 0  # "free": nothing there
    tsdf, weight = C.random_model((7, 9, 12), 21)
    d2 = E.transform(tsdf, weight, C.VOXEL, 4, unknown="occupied")[0]
    assert np.all(d2[weight == 0] == 0)


def test_degenerate_models_have_no_sites():
    for name in ("empty", "a single observed voxel"):
        tsdf, weight, kw = C.fixed_cases()[name]
        d2, nearest, esdf, record = E.transform(tsdf, weight, C.VOXEL, **kw)
        assert record == {"sites": 0, "finite": 0, "max_distance2": 0}
        assert np.all(d2 == FAR) and np.all(nearest == -1)
        want = np.full(tsdf.shape, np.float32(7) * np.float32(C.VOXEL), np.float32)
        if name != "empty":
            want[2, 2, 4] = -want[2, 2, 4]  # inside, and beyond the cap
        assert np.array_equal(esdf, want)


def test_sphere_scene_accuracy(sphere):
    """Measured with this restatement: 43 062 carved voxels at a mean error of 0.863 voxels (99th percentile 3.4); 19 998
    in-band voxels outside the surfaces at 0.745 voxels against 6.00 for tsdf * 0.08."""
    tsdf, weight, esdf, d2 = sphere["tsdf"], sphere["weight"], sphere["esdf"], sphere["distance2"]
    analytic = C.sphere_analytic_distance()
    carved = (weight > 0) & (tsdf == 1) & (d2 <= 16 ** 2)
    error = np.abs(esdf[carved] - analytic[carved]) / C.VOXEL
    print("carved: %d voxels, mean %.3f, 99th percentile %.2f voxels" % (carved.sum(), error.mean(),
                                                                         np.percentile(error, 99)))
    assert carved.sum() > 40000
    assert error.mean() <= 1.0  # a site's centre is within a voxel of the crossing
    band = (weight > 0) & (np.abs(tsdf) < 1) & (analytic > 0)
    field = np.abs(esdf[band] - analytic[band]) / C.VOXEL
    projective = np.abs(tsdf[band] * 0.08 - analytic[band]) / C.VOXEL
    print("in band: %d voxels, esdf mean %.3f, tsdf * 0.08 mean %.3f voxels" % (band.sum(), field.mean(),
                                                                                projective.mean()))
    assert band.sum() > 15000
    assert field.mean() < projective.mean() / 4


def test_header_binding_and_exports():
    import levelsetfusion_python_amd as lsf
    L = lsf._lib
    header = open(os.path.join(ROOT, "include", "lsf_hip.h")).read()
    p = L.EsdfParams
    assert [f[0] for f in p._fields_] == ["voxel_size", "iso", "min_weight", "depth", "height", "width",
                                          "max_distance_voxels", "unknown", "passes"]
    assert ctypes.sizeof(p) == 40 and p.iso.offset == 8 and p.depth.offset == 16 and p.passes.offset == 36
    assert "} lsf_esdf_params;" in header
    for macro, value in (("UNKNOWN_FREE", L.ESDF_UNKNOWN["free"]), ("UNKNOWN_OCCUPIED", L.ESDF_UNKNOWN["occupied"]),
                         ("PASS_X", L.ESDF_PASS_X), ("PASS_Y", L.ESDF_PASS_Y), ("PASS_Z", L.ESDF_PASS_Z),
                         ("PASSES_ALL", L.ESDF_PASSES_ALL), ("MAX_DISTANCE", L.ESDF_MAX_DISTANCE),
                         ("MAX_BLOCKS", L.ESDF_MAX_BLOCKS), ("BLOCK_ROWS", L.ESDF_BLOCK_ROWS),
                         ("BLOCK_VOXELS", L.ESDF_BLOCK_VOXELS), ("RECORD_WORDS", L.ESDF_RECORD_WORDS)):
        assert "#define LSF_ESDF_%s %d\n" % (macro, value) in header, macro
    assert "#define LSF_ESDF_FAR 0x7fffffff\n" in header and L.ESDF_FAR == FAR
    assert L.ESDF_MAX_DISTANCE == E.MAX_DISTANCE and L.ESDF_RECORD_FIELDS == E.RECORD_FIELDS
    assert tuple(L.ESDF_UNKNOWN) == E.UNKNOWN
    assert "#define LSF_ABI_VERSION 4" in header and L.ABI_VERSION == 4 and L.lib.lsf_abi_version() == 4
    assert "lsf_esdf_compute" in L.PROTOTYPES and L.lib.lsf_esdf_compute is not None and "lsf_esdf_compute" in header
    assert "lsf_esdf.hip" in lsf._build.SOURCES
    assert callable(lsf.fusion.CanonicalVolume.esdf) and callable(lsf.fusion.SequenceFusion3d.esdf)
    assert "ESDF_RECORD_FIELDS" in lsf.fusion.__all__ and lsf.fusion.ESDF_RECORD_FIELDS == E.RECORD_FIELDS
    assert "unpack_esdf_record" in lsf.fusion.__all__
    assert lsf.fusion.unpack_esdf_record([3, 2, 1]) == {"sites": 3, "finite": 2, "max_distance2": 1}
    assert "Euclidean distance field" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "Euclidean distance field" in lsf.fusion.__doc__


# a child without torch and with every GPU hidden: the entry point's own refusals are host code, and a call that a
# refusal should have stopped must find no device to launch on
_CHILD = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
count = ctypes.c_int(-1)
hidden = lib.hipGetDeviceCount(ctypes.byref(count)) != 0 or count.value == 0
fn = lib.lsf_esdf_compute
fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p] * 10
out = []
for case in json.load(sys.stdin):
    if case["passes"] and not hidden:  # never launch on made-up pointers
        out.append(None)
        continue
    params = ctypes.create_string_buffer(bytes.fromhex(case["params"])) if case["params"] else None
    out.append(fn(*case["args"], params, None))
print(json.dumps(out))
"""


def test_the_entry_point_refuses_on_its_own():
    """non-positive dimensions, R outside 1 .. 4096, a voxel_size that is not finite and positive, NaN iso or min_weight,
    an unknown code, NULLs, misalignment, overlaps.  Made-up addresses 16 MiB apart, never dereferenced: every refused
    case must return before a launch"""
    import levelsetfusion_python_amd as lsf
    L = lsf._lib
    shape = (20, 30, 40)
    volume = 4 * 20 * 30 * 40
    names = ("tsdf", "weight", "scratch_a", "scratch_b", "distance2", "nearest", "esdf", "record")
    base = {name: 0x10000000 + 0x1000000 * i for i, name in enumerate(names)}

    def params(**kw):
        p = L.EsdfParams()
        p.voxel_size, p.iso, p.min_weight = 0.004, 0.0, 0.0
        p.depth, p.height, p.width = shape
        p.max_distance_voxels, p.unknown, p.passes = 32, 0, L.ESDF_PASSES_ALL
        for k, v in kw.items():
            setattr(p, k, v)
        return bytes(p).hex()

    def call(passes=False, params_=None, no_params=False, **moved):
        at = dict(base, **moved)
        return dict(passes=passes, params=None if no_params else (params_ or params()), args=[at[n] for n in names])

    refused = {"no params": call(no_params=True)}
    for name in names:
        refused["without %s" % name] = call(**{name: None})
    for field, value in (("depth", 0), ("height", 0), ("width", 0), ("depth", -3), ("width", -1),
                         ("max_distance_voxels", 0), ("max_distance_voxels", -1), ("max_distance_voxels", 4097),
                         ("voxel_size", 0.0), ("voxel_size", -0.004), ("voxel_size", math.nan),
                         ("voxel_size", math.inf), ("iso", math.nan), ("min_weight", math.nan), ("unknown", 2),
                         ("unknown", -1), ("passes", 0), ("passes", 8)):
        refused["%s %r" % (field, value)] = call(params_=params(**{field: value}))
    refused["tsdf off alignment"] = call(tsdf=base["tsdf"] + 2)
    refused["record off alignment"] = call(record=base["record"] + 4)
    refused["scratch_a overlaps tsdf"] = call(scratch_a=base["tsdf"] + volume - 4)
    refused["scratch_b is scratch_a"] = call(scratch_b=base["scratch_a"])
    refused["distance2 overlaps weight"] = call(distance2=base["weight"] + 4)
    refused["nearest overlaps distance2"] = call(nearest=base["distance2"] + volume - 4)
    refused["esdf overlaps scratch_b"] = call(esdf=base["scratch_b"] + 8)
    refused["record inside esdf"] = call(record=base["esdf"] + 16)
    too_many = {"more than 2^31 - 1 voxels": call(params_=params(depth=2048, height=1024, width=1024))}
    passing = {"the plain call": call(passes=True),
               "R at its ends": call(passes=True, params_=params(max_distance_voxels=4096)),
               "infinite iso": call(passes=True, params_=params(iso=math.inf, min_weight=-math.inf, unknown=1)),
               "one pass": call(passes=True, params_=params(passes=L.ESDF_PASS_Y)),
               "scratch_a right behind tsdf": call(passes=True, scratch_a=base["tsdf"] + volume)}
    cases = dict(refused, **too_many, **passing)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    done = subprocess.run([sys.executable, "-c", _CHILD, L.LIB_PATH], input=json.dumps(list(cases.values())),
                          capture_output=True, text=True, env=env, timeout=120)
    assert done.returncode == 0, done.stderr
    status = dict(zip(cases, json.loads(done.stdout)))
    for name in refused:
        assert status[name] == -1, (name, status[name])
    assert status["more than 2^31 - 1 voxels"] == -2
    for name in passing:  # past every check: without a device the fill itself fails; None where a device was visible
        assert status[name] is None or status[name] not in (0, -1, -2), (name, status[name])


def test_python_refusals_come_before_the_gpu():
    import torch
    from levelsetfusion_python_amd import device_esdf as D, fusion
    good = dict(shape=(4, 5, 6), voxel_size=0.004, max_distance_voxels=8, iso=0.0, min_weight=0.0, unknown="free")
    p = D.params(**good)
    assert (p.depth, p.height, p.width, p.max_distance_voxels, p.unknown, p.passes) == (4, 5, 6, 8, 0, 7)
    assert D.params(**dict(good, unknown="occupied", max_distance_voxels=np.int64(4096))).unknown == 1
    for bad in (dict(shape=(4, 5)), dict(shape=(4, 0, 6)), dict(shape=(2048, 1024, 1024)),
                dict(max_distance_voxels=0), dict(max_distance_voxels=4097), dict(max_distance_voxels=-1),
                dict(max_distance_voxels=2.5), dict(max_distance_voxels=True), dict(max_distance_voxels=None),
                dict(unknown="solid"), dict(unknown=None), dict(unknown=1),
                dict(voxel_size=0.0), dict(voxel_size=-1.0), dict(voxel_size=math.nan), dict(voxel_size=math.inf),
                dict(iso=math.nan), dict(min_weight=math.nan), dict(passes=0), dict(passes=8)):
        with pytest.raises(ValueError):
            D.params(**dict(good, **bad))
    worker = D.Esdf()
    t, w = torch.zeros((4, 5, 6)), torch.zeros((4, 5, 6))
    for tsdf, weight, kw in ((t, w, dict(max_distance_voxels=0)), (t, w, dict(unknown="solid")),
                             (torch.zeros((5, 6)), torch.zeros((5, 6)), {}), (t, w, dict(voxel_size=math.nan))):
        with pytest.raises(ValueError):
            worker.compute(tsdf, weight, **kw)
    if not torch.cuda.is_available():  # past the checks there is no CPU path
        with pytest.raises(RuntimeError, match="no CPU execution path"):
            worker.compute(t, w)
        with pytest.raises(RuntimeError, match="no CPU execution path"):
            fusion.CanonicalVolume(8)
        return
    volume = fusion.CanonicalVolume(8)
    for kw in (dict(unknown="solid"), dict(max_distance_voxels=0), dict(max_distance_voxels=4097),
               dict(voxel_size=-0.004), dict(iso=math.nan), dict(brick_store=fusion.BrickStore()),
               dict(array_offset=np.zeros(3)), dict(brick_store="store", array_offset=np.zeros(3))):
        with pytest.raises(ValueError):
            volume.esdf(**kw)
    with pytest.raises(ValueError):
        fusion.CanonicalVolume((8, 8)).esdf()
