"""GPU checks of the ray-caster (csrc/lsf_raycast.hip: lsf_raycast, lsf_raycast_colour) at its edges, on the closed-form
scenes of tests/raycast_edge_scene.py.  Depth and hit count are compared with the unclipped brute-force march
(tests/raycast_bruteforce.py), which has no lo, hi, first step, last step or step cap: a wrong pad, a wrong b_j == 0
branch or a binding cap in the kernel cannot be wrong identically on both sides.  Normals are taken at a hit and do not
depend on the clip; they are compared with tests/raycast_restatement.py.  Everything is bit for bit.
tests/test_raycast_edges_host.py checks on the CPU that every scene reaches the edge it is named after."""
import numpy as np
import pytest
import torch

import raycast_edge_scene as ES
import raycast_restatement as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lsf():
    import levelsetfusion_python_amd as m
    return m


def _camera(K_, ratio=1.0):
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    return DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=K_), depth_unit_ratio=ratio)


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _bits_equal_but_nan_payloads(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and _bits_equal(a[~nan], b[~nan])


def _volume(lsf, case):
    vol = lsf.fusion.CanonicalVolume(case.tsdf.shape, colour=case.colour is not None)
    vol.tsdf.copy_(torch.from_numpy(case.tsdf))
    vol.weight.copy_(torch.from_numpy(case.weight))
    if case.colour is not None:
        vol.colour.copy_(torch.from_numpy(case.colour))
    return vol


def _cast(vol, case, ratio=1.0, **kwargs):
    """device_raycast.raycast of the case, as host arrays: (depth, normals or None, hits[, colour image])"""
    from levelsetfusion_python_amd import device_raycast
    out = device_raycast.raycast(vol.tsdf, vol.weight, _camera(case.K, ratio), case.twist, case.offset,
                                 voxel_size=case.voxel_size, image_shape=case.image_shape, **kwargs)
    return tuple(None if x is None else x.cpu().numpy() for x in out)


@pytest.mark.parametrize("case", ES.finite_cases(), ids=repr)
def test_depth_and_hits_equal_the_unclipped_march(lsf, case):
    """depth bits and hit count against the brute-force march, normals against the restatement, depth again without
    normals; through device_raycast.raycast and through CanonicalVolume.raycast"""
    ref = ES.reference(case)
    vol = _volume(lsf, case)
    depth, normals, hits = _cast(vol, case, normals=True)
    assert int(hits[0]) == ref.hits
    assert _bits_equal(depth, ref.depth)
    assert np.array_equal(depth > 0, ref.hit)
    assert _bits_equal(normals, ref.normals)
    assert np.array_equal(~normals.any(axis=2) & ref.hit, ref.zero_normal)  # depth kept, normal 0
    alone, none, hits = _cast(vol, case)
    assert none is None and int(hits[0]) == ref.hits and _bits_equal(alone, ref.depth)
    d, n = vol.raycast(_camera(case.K), case.twist, case.offset, voxel_size=case.voxel_size,
                       image_shape=case.image_shape, normals=True)
    assert _bits_equal(d, ref.depth) and _bits_equal(n, ref.normals)


@pytest.mark.parametrize("case", ES.crop_cases(), ids=repr)
def test_crops_and_the_hit_counter(lsf, case):
    """every image shape is the top-left crop of the brute-force 21 x 33 image; lanes of the last tile that lie
    outside the image count no hit, and a caller's counter is added to"""
    full = ES.reference(ES.ball("mixed", "ones"))
    h, w = case.image_shape
    want = int(full.hit[:h, :w].sum())
    vol = _volume(lsf, case)
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    for _ in range(2):
        depth, normals, hits = _cast(vol, case, normals=True, hit_count=count)
        assert _bits_equal(depth, full.depth[:h, :w]) and _bits_equal(normals, full.normals[:h, :w])
    assert int(count.item()) == 2 * want


@pytest.mark.parametrize("shape", [(21, 33), (7, 9)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("dtype,ratio", [(np.uint16, 0.001), (np.float32, 0.5), (np.float64, 0.25)],
                         ids=["uint16", "float32", "float64"])
def test_fallback_images_on_a_scene_of_misses(lsf, dtype, ratio, shape):
    """ball / holes / front is mostly misses: they take the scaled fallback bit for bit and their normals stay 0"""
    from levelsetfusion_python_amd.tsdf.generation import device_depth
    case = ES.ball("front", "holes", shape, name="ball/holes/front/%dx%d" % shape)
    ref = ES.reference(case)
    assert ref.hits < ref.hit.size // 2
    rng = np.random.default_rng(11)
    if dtype == np.uint16:
        fallback = rng.integers(0, 3000, shape).astype(np.uint16)
    else:
        fallback = rng.uniform(0.0, 9.0, shape).astype(dtype)
    scaled = RC._fallback(fallback, ratio)
    want = np.where(ref.hit, ref.depth, scaled).astype(np.float32)
    fb, code = device_depth(fallback)
    vol = _volume(lsf, case)
    depth, normals, hits = _cast(vol, case, ratio, normals=True, fallback_depth=fb, fallback_code=code)
    assert int(hits[0]) == ref.hits
    assert _bits_equal(depth, want) and _bits_equal(depth[~ref.hit], scaled[~ref.hit])
    assert _bits_equal(normals, ref.normals) and not normals[~ref.hit].any()


@pytest.mark.parametrize("case", ES.colour_cases(), ids=repr)
def test_colour_image_at_the_unclipped_hit_points(lsf, case):
    """lsf_raycast_colour: depth, normals and hits equal lsf_raycast's bit for bit; (R, G, B, Y) equals the restated
    colour step at the brute-force march's s_hit; four NaNs without a hit or without a valid colour sample"""
    ref = ES.reference(case)
    want, valid = ES.colour_reference(case)
    vol = _volume(lsf, case)
    plain_d, plain_n, plain_h = _cast(vol, case, normals=True)
    depth, normals, hits, image = _cast(vol, case, normals=True, colour=vol.colour)
    assert int(hits[0]) == int(plain_h[0]) == ref.hits
    assert _bits_equal(depth, plain_d) and _bits_equal(normals, plain_n) and _bits_equal(depth, ref.depth)
    assert np.array_equal(np.isnan(image).all(axis=2), ~valid) and np.array_equal(np.isnan(image).any(axis=2), ~valid)
    assert _bits_equal(image[valid], want[valid])
    d, n, c = vol.raycast(_camera(case.K), case.twist, case.offset, voxel_size=case.voxel_size,
                          image_shape=case.image_shape, normals=True, colours=True)
    assert _bits_equal(d, ref.depth) and _bits_equal(c[valid], want[valid]) and np.isnan(c[~valid]).all()


@pytest.mark.parametrize("case", ES.nonfinite_cases(), ids=repr)
def test_a_non_finite_tsdf_propagates_into_the_image(lsf, case):
    """validity is a matter of weights only: a NaN or an infinite tsdf under a positive weight is sampled, and the
    kernel equals the restatement in the hit mask, the hit count, the positions of NaN depths and normals and every
    other bit.  NaN payloads are not compared"""
    ref = ES.reference(case)
    vol = _volume(lsf, case)
    depth, normals, hits = _cast(vol, case, normals=True)
    assert int(hits[0]) == ref.restated_hits == ref.hits
    assert _bits_equal_but_nan_payloads(depth, ref.restated_depth)
    assert _bits_equal_but_nan_payloads(depth, ref.depth)
    assert _bits_equal_but_nan_payloads(normals, ref.normals)


def test_reruns_are_bit_identical(lsf):
    case = ES.colour_cases()[-1]
    vol = _volume(lsf, case)
    first = _cast(vol, case, normals=True, colour=vol.colour)
    again = _cast(vol, case, normals=True, colour=vol.colour)
    for a, b in zip(first, again):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
