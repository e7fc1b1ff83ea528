"""GPU checks of the Euclidean distance field: lsf_esdf_compute (csrc/lsf_esdf.hip) against the numpy restatement
(tests/esdf_restatement.py) exactly -- distance2, nearest, the bits of esdf and the record -- on ragged non-cubic
volumes, rows wider than any chunk of 64 voxels, the fixed inputs of the CPU suite, a volume that takes every capped
grid into its second trip, a rerun, and through CanonicalVolume.esdf and SequenceFusion3d.esdf.
The x pass sweeps a row in chunks of 64 voxels with a carried nearest site: X = 300 has five chunks, the last ragged,
and at R = 40 with sparse sites the nearest site of most voxels lies in another chunk.  X = 3, 4 and 9 leave most of a
chunk's lanes idle.  The y and z passes walk outwards to min(R, the farther face): R = 1, R inside the extent and R
beyond every extent take the three forms of that bound."""
import numpy as np
import pytest
import torch

import esdf_cases as C
import esdf_restatement as E
import fusion_scene as S
import moving_volume_scene as MS

pytestmark = pytest.mark.gpu

GARBAGE = 0x5a5a5a5a  # what the outputs hold before a call: every word must be written


@pytest.fixture(scope="module")
def lsf():
    import levelsetfusion_python_amd as m
    return m


@pytest.fixture(scope="module")
def worker(lsf):
    from levelsetfusion_python_amd import device_esdf
    return device_esdf.Esdf()


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the shared models are read only


def _run(worker, tsdf, weight, **kw):
    """(distance2, nearest, esdf, record) of the device call on outputs that held garbage, as host arrays"""
    outputs = tuple(torch.full(tsdf.shape, GARBAGE, dtype=torch.int32, device="cuda") for _ in range(3))
    outputs = (outputs[0], outputs[1], outputs[2].view(torch.float32))
    esdf, distance2, nearest, record = worker.compute(_dev(tsdf), _dev(weight), C.VOXEL, outputs=outputs, **kw)
    return distance2.cpu().numpy(), nearest.cpu().numpy(), esdf.cpu().numpy(), record


def _same(got, want):
    """exact equality of (distance2, nearest, esdf, record), the bits of esdf included (-0.0 is not +0.0 here)"""
    assert np.array_equal(got[0], want[0]), "distance2"
    assert np.array_equal(got[1], want[1]), "nearest"
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), "esdf"
    assert got[3] == want[3]


def _check(worker, tsdf, weight, **kw):
    want = E.transform(tsdf, weight, C.VOXEL, **kw)
    _same(_run(worker, tsdf, weight, **kw), want)
    return want


@pytest.mark.parametrize("radius", (1, 5, 64))
@pytest.mark.parametrize("shape", ((9, 21, 37), (37, 9, 21)))
def test_ragged_non_cubic(worker, shape, radius):
    tsdf, weight = C.random_model(shape, 3)
    want = _check(worker, tsdf, weight, max_distance_voxels=radius)
    assert want[3]["sites"] > 1000 and want[3]["finite"] > want[3]["sites"]


@pytest.mark.parametrize("shape,seed", (((3, 4, 300), 31), ((300, 3, 4), 31), ((4, 300, 3), 30)))
def test_wide_row_with_sparse_sites(worker, shape, seed):
    tsdf, weight = C.random_model(shape, seed, observed=0.02)
    want = _check(worker, tsdf, weight, max_distance_voxels=40)
    # the premise: a few sites, windows that run their whole length, voxels at the cap itself and voxels beyond it
    assert 4 <= want[3]["sites"] <= 8 and want[3]["max_distance2"] == 40 ** 2
    assert 1000 < want[3]["finite"] < tsdf.size - 1000


@pytest.mark.parametrize("name", list(C.fixed_cases()))
def test_fixed_inputs(worker, name):
    tsdf, weight, kw = C.fixed_cases()[name]
    _check(worker, tsdf, weight, **kw)


def test_the_capped_grids_take_a_second_trip(lsf, worker):
    """Every launch walks a grid capped at LSF_ESDF_MAX_BLOCKS = 2048 workgroups ("Capped grids and the tests
    that cross them").  The x pass gives a wave a row: 2048 * LSF_ESDF_BLOCK_ROWS = 8192 rows per trip, and (40, 256, 64)
    has 40 * 256 = 10240.  The y and z passes give a lane a voxel: 2048 * LSF_ESDF_BLOCK_VOXELS = 524288 voxels per trip,
    and the volume has 655360 (2.6 MB a buffer).  Both second trips begin at z = 32.  At R = 4 a site reaches a box of 9^3
    voxels, so the restatement's brute force covers the whole volume in well under a second."""
    L = lsf._lib
    shape = (40, 256, 64)
    per_trip = L.ESDF_MAX_BLOCKS * L.ESDF_BLOCK_VOXELS
    assert shape[0] * shape[1] > L.ESDF_MAX_BLOCKS * L.ESDF_BLOCK_ROWS == 32 * shape[1]
    assert int(np.prod(shape)) > per_trip == 32 * shape[1] * shape[2]
    tsdf, weight = C.random_model(shape, 7, observed=0.05)
    want = _check(worker, tsdf, weight, max_distance_voxels=4)
    second = want[0].ravel()[per_trip:]
    assert E.sites(tsdf, weight).ravel()[per_trip:].sum() > 500
    assert (second != E.INT32_MAX).sum() > 50000 and (second == E.INT32_MAX).sum() > 50000
    assert 0 < want[3]["finite"] < tsdf.size


def test_a_rerun_is_bit_identical(worker):
    tsdf, weight = C.random_model((21, 37, 70), 9, observed=0.1)
    first = _run(worker, tsdf, weight, max_distance_voxels=9)
    again = _run(worker, tsdf, weight, max_distance_voxels=9)
    _same(again, first)
    _same(first, E.transform(tsdf, weight, C.VOXEL, 9))


# ---- the public interface ---------------------------------------------------------------------------------------------------

def _camera(K):
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    return DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=K), depth_unit_ratio=1.0)


def test_canonical_volume_esdf_on_the_sphere_model(lsf):
    tsdf, weight = C.sphere_model()
    volume = lsf.fusion.CanonicalVolume(C.SPHERE_N)
    volume.tsdf.copy_(_dev(tsdf))
    volume.weight.copy_(_dev(weight))
    want = E.transform(tsdf, weight, C.VOXEL, 16)
    esdf, nearest = volume.esdf(C.VOXEL, 16, nearest=True)
    assert isinstance(esdf, np.ndarray) and esdf.dtype == np.float32 and nearest.dtype == np.int32
    assert np.array_equal(esdf.view(np.uint32), want[2].view(np.uint32)) and np.array_equal(nearest, want[1])
    assert volume.last_esdf_record == want[3] and volume.last_esdf_offset is None
    alone = volume.esdf(C.VOXEL, 16)
    assert isinstance(alone, np.ndarray) and np.array_equal(alone.view(np.uint32), esdf.view(np.uint32))
    t_esdf, t_nearest = volume.esdf(C.VOXEL, 16, nearest=True, as_tensor=True)
    assert t_esdf.is_cuda and t_nearest.is_cuda and t_esdf.dtype == torch.float32 and t_nearest.dtype == torch.int32
    assert np.array_equal(t_esdf.cpu().numpy().view(np.uint32), esdf.view(np.uint32))
    assert np.array_equal(t_nearest.cpu().numpy(), nearest)
    # the other keywords reach the kernel
    occupied = volume.esdf(C.VOXEL, 5, iso=0.1, min_weight=1.0, unknown="occupied")
    want = E.transform(tsdf, weight, C.VOXEL, 5, iso=0.1, min_weight=1.0, unknown="occupied")
    assert np.array_equal(occupied.view(np.uint32), want[2].view(np.uint32)) and volume.last_esdf_record == want[3]
    # the model is read only
    assert np.array_equal(volume.tsdf.cpu().numpy(), tsdf) and np.array_equal(volume.weight.cpu().numpy(), weight)


def test_sequence_esdf_after_four_tracked_frames(lsf):
    n = 48
    seq = lsf.SequenceFusion3d(_camera(S.K), n, S.offset(n), tracking_reference="icp")
    for depth in S.frames(4):
        seq.integrate(depth)
    tsdf, weight = seq.canonical.tsdf.cpu().numpy(), seq.canonical.weight.cpu().numpy()
    want = E.transform(tsdf, weight, seq.voxel_size, 12)
    esdf, nearest = seq.esdf(12, nearest=True)
    assert np.array_equal(esdf.view(np.uint32), want[2].view(np.uint32)) and np.array_equal(nearest, want[1])
    assert seq.last_esdf_record == want[3] and want[3]["sites"] > 1000
    assert np.array_equal(seq.last_esdf_offset, seq.array_offset)
    with pytest.raises(ValueError, match="keep_tsdf"):
        seq.esdf(include_streamed=True)  # no moving volume, no brick store
    with pytest.raises(ValueError):
        seq.esdf(unknown="solid")
    with pytest.raises(ValueError):
        seq.esdf(max_distance_voxels=0)


def test_sequence_esdf_of_the_whole_map(lsf):
    """the out-and-back trajectory of tests/test_gpu_volume_bricks.py with keep_tsdf: the field of window and store is
    the restatement applied to assemble's volume"""
    from test_gpu_volume_bricks import _return_frames
    policy = lsf.fusion.MovingVolume(MS.THRESHOLD, MS.ANCHOR, stream_mesh=False, keep_tsdf=True)
    seq = lsf.SequenceFusion3d(_camera(MS.K), MS.WINDOW, MS.WINDOW_OFFSET, voxel_size=MS.VOXEL,
                               narrow_band_width_voxels=MS.BAND, tracking_reference="icp", moving_volume=policy)
    for depth in _return_frames():
        seq.integrate(depth)
    assert len(seq.brick_store) > 0
    tsdf, weight, _, offset = seq.canonical.assemble(seq.brick_store, seq.array_offset)
    tsdf, weight = tsdf.cpu().numpy(), weight.cpu().numpy()
    assert tsdf.size > MS.WINDOW ** 3
    want = E.transform(tsdf, weight, MS.VOXEL, 8)
    esdf, nearest = seq.esdf(8, nearest=True, include_streamed=True)
    assert esdf.shape == tsdf.shape
    assert np.array_equal(esdf.view(np.uint32), want[2].view(np.uint32)) and np.array_equal(nearest, want[1])
    assert seq.last_esdf_record == want[3] and np.array_equal(seq.last_esdf_offset, offset)
    window = seq.esdf(8)  # the window alone is another field: sites of the store are missing from it
    assert window.shape == (MS.WINDOW,) * 3 and seq.last_esdf_record["sites"] < want[3]["sites"]
    with pytest.raises(ValueError, match="max_voxels"):
        seq.canonical.esdf(MS.VOXEL, 8, brick_store=seq.brick_store, array_offset=seq.array_offset,
                           max_voxels=MS.WINDOW ** 3)
