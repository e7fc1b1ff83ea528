"""GPU checks of mesh simplification (csrc/lsf_mesh_simplify.hip, device_mesh_simplify.simplify, fusion.simplify_mesh)
against the numpy restatement (tests/mesh_simplify_restatement.py): vertex and normal float32 bit patterns, colours,
faces, the order of both arrays and the whole record, all exactly."""
import functools

import numpy as np
import pytest
import torch

import mesh_restatement as M
import mesh_simplify_restatement as R
import moving_volume_scene as MS

pytestmark = pytest.mark.gpu

SPHERE = (24, (11.5, 11.8, 11.3), 8.3)
NOISE_OFFSET, NOISE_VOXEL = (1.5, -2.0, 0.25), 0.01
SPHERE_CASES = ((0.5, (0, 0, 0)), (2.0, (0, 0, 0)), (2.5, (0.3, -0.7, 0.45)), (4.0, (0.3, -0.7, 0.45)),
                (30.0, (0, 0, 0)))


@pytest.fixture(scope="module")
def lsf():
    import levelsetfusion_python_amd as m
    return m


@pytest.fixture(scope="module")
def simplify():
    from levelsetfusion_python_amd import device_mesh_simplify
    return device_mesh_simplify.simplify


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


def _colours(count, seed=5):
    return np.random.default_rng(seed).integers(0, 256, (count, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _sphere_mesh(offset=(0, 0, 0), voxel=1.0):
    t = _sphere(*SPHERE)
    return M.extract(t, np.ones_like(t), list(offset), voxel, normals=True)


@functools.lru_cache(maxsize=None)
def _noise_mesh(seed):
    t = _noise((14, 14, 14), seed)
    return M.extract(t, np.ones_like(t), list(NOISE_OFFSET), NOISE_VOXEL, normals=True)


def _merge(meshes):
    """the concatenation, as fusion.merge_meshes makes it, of (V, F, N) meshes"""
    base, out_v, out_f, out_n = 0, [], [], []
    for v, f, n in meshes:
        out_v.append(v)
        out_f.append(f + base)
        out_n.append(n)
        base += len(v)
    return np.concatenate(out_v), np.concatenate(out_f).astype(np.int32), np.concatenate(out_n)


def _split(t, offset, voxel):
    """the volume cut at x-cell X // 2 into two volumes that share that layer, each meshed on its own, and merged"""
    k = t.shape[2] // 2
    w = np.ones_like(t)
    low = M.extract(t[:, :, :k + 1], w[:, :, :k + 1], list(offset), voxel, normals=True)
    high = M.extract(t[:, :, k:], w[:, :, k:], [offset[0] + k, offset[1], offset[2]], voxel, normals=True)
    return _merge([low, high])


@functools.lru_cache(maxsize=None)
def _tripled_noise():
    return _merge([_noise_mesh(0)] * 3)


def _device(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want))


def _host(out):
    return tuple(None if t is None else t.cpu().numpy() for t in out[:4]) + (out[4],)


def _check(simplify, mesh, cell=None, origin=(0, 0, 0), table_slots=None):
    """the call with and without normals and colours against the restatement; returns the restatement's result"""
    v, f, n = mesh
    c = _colours(len(v))
    want = R.simplify(v, f, n, c, cell, origin)
    got = _host(simplify(_device(v), _device(f), _device(n), _device(c), cell, origin, table_slots))
    assert got[4] == want[4], (got[4], want[4])
    for g, w, name in zip(got[:4], want[:4], ("vertices", "faces", "normals", "colours")):
        assert _same(g, w), name
    bare = _host(simplify(_device(v), _device(f), None, None, cell, origin, table_slots))
    assert bare[4] == want[4] and bare[2] is None and bare[3] is None
    assert _same(bare[0], want[0]) and _same(bare[1], want[1])  # attributes change nothing else
    return want


@pytest.mark.parametrize("cell,origin", SPHERE_CASES)
def test_sphere_clusters(simplify, cell, origin):
    want = _check(simplify, _sphere_mesh(), cell, origin)
    assert want[4]["vertices_in"] == 1288 and want[4]["faces_in"] == 2572


@pytest.mark.parametrize("seed,cell", [(0, 0.02), (0, 0.035), (1, 0.02), (1, 0.035)])
def test_padded_noise_clusters(simplify, seed, cell):
    """flaps, multiply covered triples and orphan clusters: the branches the sphere never takes"""
    details = {}
    mesh = _noise_mesh(seed)
    R.simplify(*mesh, None, cell, details=details)
    assert details["group_sizes"].max() >= 3
    want = _check(simplify, mesh, cell)
    assert want[4]["cancelled_groups"] > 0 and want[4]["orphan_clusters"] > 0


@pytest.mark.parametrize("case", ["sphere", "sphere at an offset", "noise"])
def test_seam_weld(simplify, case):
    if case == "noise":
        t, off, voxel = _noise((14, 14, 14), 0), NOISE_OFFSET, NOISE_VOXEL
    else:
        t = _sphere(*SPHERE)
        off, voxel = ((0, 0, 0), 1.0) if case == "sphere" else (NOISE_OFFSET, 0.004)
    merged = _split(t, off, voxel)
    whole = M.extract(t, np.ones_like(t), list(off), voxel)
    assert len(merged[0]) > len(whole[0]) and not M.is_closed_manifold(merged[1])
    want = _check(simplify, merged)
    assert len(want[0]) == len(whole[0]) and len(want[1]) == len(whole[1]) and M.is_closed_manifold(want[1])


def test_mirror_wound_copy_and_signed_zero(simplify):
    v, f, n = _sphere_mesh()
    both = _merge([(v, f, n), (v, np.ascontiguousarray(f[:, ::-1]), n)])
    want = _check(simplify, both)
    assert want[4]["vertices_out"] == 0 and want[4]["cancelled_groups"] == len(f) and want[0].shape == (0, 3)
    v2 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-0.0, 0, -0.0], [1, 1, 0]], np.float32)
    f2 = np.array([[0, 1, 2], [3, 4, 1]], np.int32)
    n2 = np.tile(np.array([[0, 0, 1]], np.float32), (5, 1))
    want = _check(simplify, (v2, f2, n2))
    assert want[4]["clusters"] == 4 and np.array_equal(want[1], [[0, 1, 2], [0, 3, 1]])


def test_table_size_changes_nothing(simplify):
    """probe sequences differ between the smallest table and one 16 times as large; no output may"""
    from levelsetfusion_python_amd import device_mesh_simplify as D
    mesh = _tripled_noise()
    least = D.smallest_table_slots(len(mesh[0]), len(mesh[1]))
    for cell in (None, 0.02):
        a = _check(simplify, mesh, cell, table_slots=least)
        b = _check(simplify, mesh, cell, table_slots=16 * least)
        assert a[4] == b[4]
    assert a[4]["multi_cover_groups"] > 0  # three copies of every surviving triple


def test_the_scan_loops_past_its_lanes(simplify):
    """the one capped loop ("Capped grids and the tests that cross them"): the scan workgroup of
    LSF_MESH_SIMPLIFY_SCAN_THREADS lanes walks more than that many tile counts, for the vertices, the faces and the
    clusters"""
    import levelsetfusion_python_amd._lib as L
    reach = L.MESH_SIMPLIFY_SCAN_THREADS * L.MESH_SIMPLIFY_TILE
    one = _noise_mesh(0)
    copies = reach // len(one[0]) + 1
    # the copies stand apart, so the clusters stay as many as the vertices; one more copy of the first welds onto it
    apart = [(one[0] + np.float32(0.25 * k), one[1], one[2]) for k in range(copies)]
    mesh = _merge(apart + [one])
    want = R.simplify(mesh[0], mesh[1], mesh[2], None, None)
    assert len(mesh[0]) > reach and len(mesh[1]) > reach and want[4]["clusters"] > reach  # it crosses
    assert want[4]["faces_out"] > reach and want[4]["multi_cover_groups"] == len(one[1])
    got = _host(simplify(_device(mesh[0]), _device(mesh[1]), _device(mesh[2]), None))
    assert got[4] == want[4]
    assert all(_same(g, w) for g, w in zip(got[:3], want[:3]))


def _volume(lsf, t):
    vol = lsf.fusion.CanonicalVolume(t.shape)
    vol.tsdf.copy_(torch.from_numpy(t))
    vol.weight.fill_(1.0)
    return vol


def test_extract_mesh_with_a_simplify_cell(lsf):
    t = _sphere(*SPHERE)
    vol = _volume(lsf, t)
    raw = vol.extract_mesh([0, 0, 0], 1.0, normals=True)
    got = vol.extract_mesh([0, 0, 0], 1.0, normals=True, simplify_cell=2.0)
    want = lsf.fusion.simplify_mesh(raw, 2.0, return_record=True)
    assert all(_same(g, w) for g, w in zip(got, want[:3])) and vol.mesh_record == want[3]
    ref = R.simplify(*raw, None, 2.0)
    assert _same(got[0], ref[0]) and _same(got[1], ref[1]) and _same(got[2], ref[2]) and want[3] == ref[4]
    assert len(got[0]) == 282 and len(got[1]) == 560
    tensors = vol.extract_mesh([0, 0, 0], 1.0, as_tensor=True, simplify_cell=2.0)
    assert len(tensors) == 2 and tensors[0].is_cuda and _same(tensors[1].cpu().numpy(), ref[1])
    plain = vol.extract_mesh([0, 0, 0], 1.0, normals=True)
    assert all(_same(a, b) for a, b in zip(plain, raw)) and vol.mesh_record is None  # the default is today's call


def test_merge_meshes_welds(lsf):
    t = _noise((14, 14, 14), 0)
    k = t.shape[2] // 2
    low = _volume(lsf, np.ascontiguousarray(t[:, :, :k + 1])).extract_mesh(list(NOISE_OFFSET), NOISE_VOXEL)
    off = [NOISE_OFFSET[0] + k, NOISE_OFFSET[1], NOISE_OFFSET[2]]
    high = _volume(lsf, np.ascontiguousarray(t[:, :, k:])).extract_mesh(off, NOISE_VOXEL)
    whole = _volume(lsf, t).extract_mesh(list(NOISE_OFFSET), NOISE_VOXEL)
    loose = lsf.fusion.merge_meshes([low, high])
    welded = lsf.fusion.merge_meshes([low, high], weld=True)
    assert len(loose[0]) > len(whole[0]) and not M.is_closed_manifold(loose[1])
    assert len(welded[0]) == len(whole[0]) == 2820 and len(welded[1]) == len(whole[1]) == 5832
    rows = lambda v: {tuple(r) for r in _bits(v).tolist()}
    assert rows(welded[0]) == rows(whole[0]) and M.is_closed_manifold(welded[1])


def test_a_streaming_sequence_welds_its_seams(lsf, capsys):
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    cam = DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=MS.K), depth_unit_ratio=1.0)
    policy = lsf.fusion.MovingVolume(MS.THRESHOLD, MS.ANCHOR)
    seq = lsf.SequenceFusion3d(cam, MS.WINDOW, MS.WINDOW_OFFSET, voxel_size=MS.VOXEL,
                               narrow_band_width_voxels=MS.BAND, tracking_reference="icp", moving_volume=policy)
    for k in range(MS.FRAMES):
        if seq.integrate(MS.render(MS.true_twist(k)))["shift"] != (0, 0, 0):
            break
    assert len(seq.streamed_meshes) >= 1 and k < 12  # it shifted once, early
    loose = seq.extract_mesh(include_streamed=True)
    welded = seq.extract_mesh(include_streamed=True, weld=True)
    rec = seq.mesh_records["weld"]
    edges = len(M.boundary_edges(loose[1])), len(M.boundary_edges(welded[1]))
    with capsys.disabled():
        print("\nstreaming run of %d frames: %d -> %d vertices, %d -> %d faces, boundary edges %d -> %d, record %r"
              % (k + 1, len(loose[0]), len(welded[0]), len(loose[1]), len(welded[1]), edges[0], edges[1], rec))
    assert len(welded[0]) < len(loose[0]) and edges[1] <= edges[0]
    assert rec["multi_cover_groups"] == 0  # then every group holds one face, or two that cancel
    assert len(welded[1]) == len(loose[1]) - rec["degenerate_faces"] - 2 * rec["cancelled_groups"] == rec["faces_out"]
    with pytest.raises(ValueError, match="weld"):
        seq.extract_mesh(weld=True)
    coarse = seq.extract_mesh(include_streamed=True, weld=True, simplify_cell=2 * MS.VOXEL)
    want = R.simplify(welded[0], welded[1], None, None, 2 * MS.VOXEL)
    assert _same(coarse[0], want[0]) and _same(coarse[1], want[1]) and seq.mesh_records["simplify"] == want[4]


def test_refusals_that_need_the_card(simplify):
    v, f, n = _sphere_mesh()
    bad = v.copy()
    bad[17, 1] = np.nan
    with pytest.raises(ValueError, match="1 vertices"):
        simplify(_device(bad), _device(f))
    with pytest.raises(ValueError, match="1 vertices"):
        simplify(_device(bad), _device(f), cell_size=2.0)
    for index in (len(v), -1):  # the two that prove the check without reaching outside the allocation without it
        faces = f.copy()
        faces[100, 2] = index
        with pytest.raises(ValueError, match="1 faces"):
            simplify(_device(v), _device(faces), _device(n), cell_size=2.0)
    far = v.copy()
    far[3, 0] = 3.0e6  # cell 2^20 + ... at cell_size 2: beyond the lattice
    with pytest.raises(ValueError, match="1 vertices"):
        simplify(_device(far), _device(f), cell_size=2.0)
    assert simplify(_device(far), _device(f))[4]["vertices_out"] == len(v)  # welding has no lattice


def test_empty_inputs(simplify):
    v, f, n = _sphere_mesh()
    none_v, none_f = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    for vertices, faces, normals in ((none_v, none_f, None), (v, none_f, n), (v, none_f, None)):
        for cell in (None, 2.0):
            want = R.simplify(vertices, faces, normals, None, cell)
            got = _host(simplify(_device(vertices), _device(faces), _device(normals), None, cell))
            assert got[4] == want[4] and got[4]["orphan_clusters"] == got[4]["clusters"]
            assert got[0].shape == (0, 3) and got[1].shape == (0, 3) and (normals is None or got[2].shape == (0, 3))
    with pytest.raises(ValueError, match="3 faces"):
        simplify(_device(none_v), _device(f[:3].copy()))  # faces without vertices: every index is outside
