"""GPU checks of mesh extraction (csrc/lsf_mesh.hip, fusion.CanonicalVolume.extract_mesh) against the numpy restatement
(tests/mesh_restatement.py): vertex and normal float32 bit patterns, faces, and the order of both arrays."""
import numpy as np
import pytest
import torch

import fusion_restatement as F
import fusion_scene as S
import mesh_restatement as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lsf():
    import levelsetfusion_python_amd as m
    return m


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _volume(lsf, t, w):
    vol = lsf.fusion.CanonicalVolume(t.shape)
    vol.tsdf.copy_(torch.from_numpy(np.ascontiguousarray(t, np.float32)))
    vol.weight.copy_(torch.from_numpy(np.ascontiguousarray(w, np.float32)))
    return vol


def _sphere(n, centre, radius, band=3.0):
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")
    d = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius
    return np.clip(d / band, -1, 1).astype(np.float32)


def _noise(shape, seed):
    t = np.random.default_rng(seed).uniform(-1, 1, shape).astype(np.float32)
    t[0] = t[-1] = 1
    t[:, 0] = t[:, -1] = 1
    t[:, :, 0] = t[:, :, -1] = 1
    return t


def _fused(n, frames=3):
    off = S.offset(n)
    t, w = F.empty_model((n,) * 3)
    for k, depth in enumerate(S.frames(frames)):
        t, w, _ = F.fuse_depth(t, w, depth, S.K, 1.0, off, S.true_twist(k))
    return t, w, off


def _check(lsf, t, w, off, voxel_size=0.004, iso=0.0, min_weight=0.0, min_faces=1):
    vol = _volume(lsf, t, w)
    verts, faces, normals = vol.extract_mesh(off, voxel_size, iso, min_weight, normals=True)
    want_v, want_f, want_n = M.extract(t, w, off, voxel_size, iso, min_weight, normals=True)
    assert faces.dtype == np.int32 and verts.dtype == np.float32 and normals.dtype == np.float32
    assert len(want_f) >= min_faces
    assert _bits_equal(verts, want_v)
    assert _bits_equal(normals, want_n)
    assert np.array_equal(faces, want_f)
    alone_v, alone_f = vol.extract_mesh(off, voxel_size, iso, min_weight)
    assert _bits_equal(alone_v, want_v) and np.array_equal(alone_f, want_f)  # normals change nothing else
    return verts, faces, normals


def test_sphere(lsf):
    t = _sphere(24, (11.5, 11.8, 11.3), 8.3)
    verts, faces, _ = _check(lsf, t, np.ones_like(t), [0, 0, 0], 1.0, min_faces=1000)
    assert M.is_closed_manifold(faces) and M.euler_characteristic(len(verts), faces) == 2


@pytest.mark.parametrize("seed", range(3))
def test_padded_noise(lsf, seed):
    """every case, ambiguous faces included; the mesh is a closed oriented 2-manifold"""
    t = _noise((14, 14, 14), seed)
    verts, faces, _ = _check(lsf, t, np.ones_like(t), [1.5, -2.0, 0.25], 0.01, min_faces=1000)
    assert M.is_closed_manifold(faces)
    assert np.array_equal(np.unique(faces), np.arange(len(verts)))  # no orphan vertices
    assert len(_cases(t)) >= 200


def _cases(t):
    """the cases of the cells of a volume of weight 1"""
    inside = (t < 0).astype(np.int64)
    case = np.zeros(tuple(v - 1 for v in t.shape), np.int64)
    for c in range(8):
        x, y, z = c & 1, (c >> 1) & 1, c >> 2
        case |= inside[z:z + case.shape[0], y:y + case.shape[1], x:x + case.shape[2]] << c
    return set(case.reshape(-1).tolist())


def test_fused_scene(lsf):
    t, w, off = _fused(48)
    verts, faces, normals = _check(lsf, t, w, off, min_faces=1000)
    assert np.all(np.abs(np.linalg.norm(normals, axis=1) - 1) < 1e-5)


def test_non_cubic_volume_with_unusable_voxels(lsf):
    shape = (40, 33, 57)
    z, y, x = np.meshgrid(*(np.arange(v, dtype=np.float64) for v in shape), indexing="ij")
    d = np.sqrt(((x - 28.2) / 1.6) ** 2 + (y - 16.1) ** 2 + (z - 19.7) ** 2) - 11.0
    t = np.clip(d / 4, -1, 1).astype(np.float32)
    w = np.random.default_rng(7).uniform(0.0, 3.0, shape).astype(np.float32)
    w[w < 0.1] = 0.0
    w[5, 16, :] = np.nan
    t[30, 10:20, 20] = np.nan
    t[12, 5, 30:40] = np.inf
    _check(lsf, t, w, [-28.0, -16.5, 100.25], 0.004, min_faces=1000)


def test_iso_level(lsf):
    t = _sphere(24, (11.5, 11.8, 11.3), 8.3)
    _check(lsf, t, np.ones_like(t), [0, 0, 0], 1.0, iso=0.25, min_faces=1000)


def test_min_weight_on_a_three_frame_model(lsf):
    t, w, off = _fused(48)
    assert np.any((w > 0) & (w <= 1.5)) and np.any(w > 1.5)
    verts, faces, _ = _check(lsf, t, w, off, min_weight=1.5, min_faces=100)
    all_v, all_f = M.extract(t, w, off)[:2]
    assert len(faces) < len(all_f)


def test_empty_model(lsf):
    vol = lsf.fusion.CanonicalVolume((16, 16, 16))
    verts, faces = vol.extract_mesh(S.offset(16))
    assert verts.shape == (0, 3) and faces.shape == (0, 3) and verts.dtype == np.float32 and faces.dtype == np.int32
    v, f, n = vol.extract_mesh(S.offset(16), normals=True, as_tensor=True)
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and tuple(n.shape) == (0, 3)


def test_minimal_volume(lsf):
    t = np.array([[[-0.5, 0.5], [0.25, 0.75]], [[0.1, -0.2], [0.6, 0.3]]], np.float32)
    _check(lsf, t, np.ones_like(t), [0, 0, 0], 1.0)


def test_gpu_mesh_is_a_watertight_sphere(lsf):
    n = 40
    t = _sphere(n, (19.6, 19.3, 20.2), 13.7)
    vol = _volume(lsf, t, np.ones_like(t))
    verts, faces = vol.extract_mesh([0, 0, 0], 1.0)
    assert M.is_closed_manifold(faces) and M.euler_characteristic(len(verts), faces) == 2
    torus = np.zeros((n, n, n), np.float32)
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")
    q = np.sqrt((x - 19.6) ** 2 + (y - 20.3) ** 2) - 11.0
    torus[:] = np.clip((np.sqrt(q ** 2 + (z - 19.8) ** 2) - 4.5) / 3, -1, 1)
    vol = _volume(lsf, torus, np.ones_like(torus))
    verts, faces = vol.extract_mesh([0, 0, 0], 1.0)
    assert M.is_closed_manifold(faces) and M.euler_characteristic(len(verts), faces) == 0


def test_two_calls_give_identical_bits(lsf):
    t, w, off = _fused(48)
    vol = _volume(lsf, t, w)
    a = vol.extract_mesh(off, normals=True)
    b = vol.extract_mesh(off, normals=True)
    assert all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                              y.view(np.uint32) if y.dtype == np.float32 else y) for x, y in zip(a, b))


def test_as_tensor_returns_device_tensors(lsf):
    t = _sphere(24, (11.5, 11.8, 11.3), 8.3)
    vol = _volume(lsf, t, np.ones_like(t))
    v, f, n = vol.extract_mesh([0, 0, 0], 1.0, normals=True, as_tensor=True)
    assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in (v, f, n))
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and n.dtype == torch.float32
    want_v, want_f, _ = M.extract(t, np.ones_like(t), [0, 0, 0], 1.0)
    assert _bits_equal(v.cpu().numpy(), want_v) and np.array_equal(f.cpu().numpy(), want_f)


def test_a_2d_model_is_refused(lsf):
    vol = lsf.fusion.CanonicalVolume((16, 16))
    with pytest.raises(ValueError, match="3-D"):
        vol.extract_mesh([0, 0, 0])


def test_bad_arguments_are_refused(lsf):
    from levelsetfusion_python_amd import device_mesh
    t = torch.zeros((4, 4, 4), device="cuda")
    with pytest.raises(ValueError, match="shape"):
        device_mesh.extract_mesh(t, torch.zeros((4, 4, 5), device="cuda"), [0, 0, 0])
    with pytest.raises(ValueError, match="float32"):
        device_mesh.extract_mesh(t, torch.zeros((4, 4, 4), dtype=torch.float64, device="cuda"), [0, 0, 0])
    vol = lsf.fusion.CanonicalVolume((4, 4, 4))
    for kw in (dict(voxel_size=0.0), dict(iso=float("nan")), dict(array_offset=[0, float("inf"), 0])):
        args = dict(array_offset=[0, 0, 0])
        args.update(kw)
        with pytest.raises(ValueError):
            vol.extract_mesh(**args)


def test_sequence_extract_mesh(lsf):
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    cam = DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=S.K), depth_unit_ratio=1.0)
    n = 32
    seq = lsf.fusion.SequenceFusion3d(cam, n, S.offset(n), voxel_size=0.004, rigid_iterations=0)
    for depth in S.frames(2):
        seq.integrate(depth)
    got = seq.extract_mesh(normals=True)
    want = seq.canonical.extract_mesh(S.offset(n), 0.004, normals=True)
    assert len(got[1]) > 100
    assert _bits_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and _bits_equal(got[2], want[2])
    t, w = seq.canonical.tsdf.cpu().numpy(), seq.canonical.weight.cpu().numpy()
    rv, rf, rn = M.extract(t, w, S.offset(n), 0.004, normals=True)
    assert _bits_equal(got[0], rv) and np.array_equal(got[1], rf) and _bits_equal(got[2], rn)
