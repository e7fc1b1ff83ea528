"""GPU checks of mesh components (csrc/lsf_mesh_components.hip, device_mesh_components, fusion.mesh_components and
fusion.filter_mesh_components) against the numpy restatement (tests/mesh_components_restatement.py): the labels, the
table, the order of both output arrays, the bit patterns of positions, normals and colours and the whole record, all
exactly."""
import numpy as np
import pytest
import torch

import mesh_components_restatement as R
import mesh_components_scenes as S
import mesh_restatement as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lsf():
    import levelsetfusion_python_amd as m
    return m


@pytest.fixture(scope="module")
def D():
    from levelsetfusion_python_amd import device_mesh_components
    return device_mesh_components


def _device(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want))


def _host(out):
    return tuple(None if t is None else t.cpu().numpy() for t in out[:4]) + (out[4],)


def _check_components(D, v, f, max_blocks=None):
    """components() against the restatement; returns the restatement's result"""
    want = R.components(v, f)
    vertex_labels, face_labels, table = D.components(_device(v), _device(f), max_blocks)
    assert _same(vertex_labels.cpu().numpy(), want[0]) and _same(face_labels.cpu().numpy(), want[1])
    assert tuple(table) == R.TABLE_FIELDS
    for name in R.TABLE_FIELDS:
        assert _same(table[name].cpu().numpy(), want[2][name]), name
    return want


def _check_filter(D, mesh, max_blocks=None, **criteria):
    """filter() with and without normals and colours against the restatement; returns the restatement's result"""
    v, f, n = mesh
    c = S.colours(len(v))
    want = R.filter(v, f, n, c, **criteria)
    got = _host(D.filter(_device(v), _device(f), _device(n), _device(c), max_blocks=max_blocks, **criteria))
    assert got[4] == want[4], (got[4], want[4])
    for g, w, name in zip(got[:4], want[:4], ("vertices", "faces", "normals", "colours")):
        assert _same(g, w), name
    bare = _host(D.filter(_device(v), _device(f), max_blocks=max_blocks, **criteria))
    assert bare[4] == want[4] and bare[2] is None and bare[3] is None
    assert _same(bare[0], want[0]) and _same(bare[1], want[1])  # attributes change nothing else
    return want


def test_floaters_scene(D):
    v, f, n = S.floaters_mesh()
    assert (len(v), len(f)) == (830, 1644)
    want = _check_components(D, v, f)
    assert tuple(want[2]["labels"]) == (0, 34, 360, 782)
    assert tuple(want[2]["vertex_counts"]) == (34, 738, 10, 48) and tuple(want[2]["face_counts"]) == (64, 1472, 16, 92)
    largest = _check_filter(D, (v, f, n), keep_largest=1)
    assert len(largest[0]) == 738 and len(largest[1]) == 1472 and M.is_closed_manifold(largest[1])
    assert len(largest[0]) - 3 * len(largest[1]) // 2 + len(largest[1]) == 2  # Euler characteristic 2
    assert _check_filter(D, (v, f, n), min_faces=64)[4]["components_kept"] == 3
    assert _check_filter(D, (v, f, n), min_faces=65)[4]["components_kept"] == 2
    extent = _check_filter(D, (v, f, n), min_extent=4.0)  # the sphere spans 12.5 voxels, the largest blob 3.2
    assert extent[4]["components_kept"] == 1 and _same(extent[1], largest[1])
    assert _check_filter(D, (v, f, n), min_vertices=11, keep_largest=2)[4]["vertices_out"] == 738 + 48
    assert _check_filter(D, (v, f, n), min_faces=2000)[4]["vertices_out"] == 0


def test_noise_mesh(D):
    v, f, n = S.noise_mesh(0)
    want = _check_components(D, v, f)
    assert (len(v), len(f), len(want[2]["labels"]), want[2]["vertex_counts"].max()) == (2820, 5832, 29, 2608)
    assert _check_filter(D, (v, f, n), keep_largest=1)[4]["vertices_out"] == 2608
    assert _check_filter(D, (v, f, n), min_faces=9, keep_largest=5)[4]["components_kept"] == 5  # ties at 16 faces
    assert 0 < _check_filter(D, (v, f, n), min_extent=1.5 * S.NOISE_VOXEL)[4]["components_kept"] < 29


def test_adversarial_union_find(D):
    """deep walks (a strip numbered at random), the minimum at the far end (a strip numbered backwards), every lane at
    one root (a fan), isolated vertices and degenerate faces, each over many workgroups"""
    v, f, parts = S.adversarial_mesh()
    want = _check_components(D, v, f)
    assert len(want[2]["labels"]) == sum(parts.values()) and want[2]["vertex_counts"].max() == 20000
    n = np.random.default_rng(2).standard_normal(v.shape).astype(np.float32)
    assert _check_filter(D, (v, f, n), keep_largest=2)[4]["vertices_out"] == 40000
    assert _check_filter(D, (v, f, n), min_faces=1, min_vertices=2)[4]["components_kept"] == 3 + parts["twice"]
    assert _check_filter(D, (v, f, n), min_vertices=1, keep_largest=4000)[4]["components_kept"] == 4000


def test_the_capped_loops_are_crossed(D):
    """every capped grid and the one-workgroup scan ("Capped grids and the tests that cross them"): more tiles
    of vertices and of faces than LSF_MESH_COMPONENTS_MAX_BLOCKS workgroups, more tile counts than the scan's
    LSF_MESH_COMPONENTS_SCAN_THREADS lanes, and more components than either reaches, for the table and the filter"""
    import levelsetfusion_python_amd._lib as L
    tile = L.MESH_COMPONENTS_TILE
    reach = max(L.MESH_COMPONENTS_MAX_BLOCKS, L.MESH_COMPONENTS_SCAN_THREADS) * tile
    v, f, components = S.crossing_mesh(reach)
    assert len(v) > reach and len(f) > reach and components > reach  # it crosses
    want = _check_components(D, v, f)
    assert len(want[2]["labels"]) == components
    n = np.ascontiguousarray(v[:, ::-1])
    kept = _check_filter(D, (v, f, n), min_vertices=1, keep_largest=reach + 2)  # the kept rows cross as well
    assert kept[4]["components_kept"] == reach + 2 and kept[4]["vertices_out"] > reach and kept[4]["faces_out"] > reach


def test_reruns_and_launch_shapes_change_nothing(D):
    v, f, _ = S.adversarial_mesh()
    n = np.random.default_rng(2).standard_normal(v.shape).astype(np.float32)
    dv, df, dn = _device(v), _device(f), _device(n)
    runs, records = [], []
    for max_blocks in (None, None, 1, 7, 64):  # two runs of the library's grid, then three other launch shapes
        labels = D.components(dv, df, max_blocks)
        kept = D.filter(dv, df, dn, None, min_faces=1, keep_largest=300, max_blocks=max_blocks)
        arrays = [labels[0], labels[1]] + [labels[2][k] for k in R.TABLE_FIELDS] + list(kept[:3])
        runs.append([t.cpu().numpy() for t in arrays])
        records.append(kept[4])
    for other, record in zip(runs[1:], records[1:]):
        assert all(_same(a, b) for a, b in zip(runs[0], other)) and record == records[0]
    _check_filter(D, (v, f, n), max_blocks=3, min_faces=1, keep_largest=300)


def test_welding_joins_what_a_seam_splits(lsf):
    low, high, whole = S.split_noise()
    loose = lsf.fusion.merge_meshes([low, high])
    welded = lsf.fusion.merge_meshes([low, high], weld=True)
    table = {}
    for name, mesh in (("loose", loose), ("welded", welded), ("whole", whole)):
        labels = lsf.fusion.mesh_components(mesh)
        want = R.components(mesh[0], mesh[1])
        assert _same(labels[0], want[0]) and _same(labels[1], want[1])
        assert all(_same(labels[2][k], want[2][k]) for k in R.TABLE_FIELDS)
        table[name] = labels[2]
    assert len(table["loose"]["labels"]) > len(table["whole"]["labels"]) == 29  # the seam splits components
    sizes = lambda t: sorted(zip(t["vertex_counts"].tolist(), t["face_counts"].tolist()))
    assert len(table["welded"]["labels"]) == 29 and sizes(table["welded"]) == sizes(table["whole"])
    bounds = lambda t: sorted(_bits(t["bounds"]).reshape(-1, 6).tolist())
    assert bounds(table["welded"]) == bounds(table["whole"])  # the same table up to the numbering of the vertices


def test_attributes_and_tensors(lsf):
    v, f, n = S.floaters_mesh()
    c = S.colours(len(v))
    want = R.filter(v, f, n, c, min_faces=17)
    got = lsf.fusion.filter_mesh_components((v, f, n, c), min_faces=17, return_record=True)
    assert all(_same(g, w) for g, w in zip(got[:4], want[:4])) and got[4] == want[4]
    assert len(lsf.fusion.filter_mesh_components((v, f, c), min_faces=17)) == 3
    assert _same(lsf.fusion.filter_mesh_components((v, f, c), min_faces=17)[2], want[3])
    tensors = lsf.fusion.filter_mesh_components((_device(v), _device(f), _device(n), _device(c)), min_faces=17,
                                                as_tensor=True)
    assert len(tensors) == 4 and all(t.is_cuda for t in tensors)
    assert all(_same(t.cpu().numpy(), w) for t, w in zip(tensors, want[:4]))
    labels = lsf.fusion.mesh_components((_device(v), _device(f)), as_tensor=True)
    assert labels[0].is_cuda and labels[1].is_cuda and all(t.is_cuda for t in labels[2].values())
    ref = R.components(v, f)
    assert _same(labels[0].cpu().numpy(), ref[0]) and _same(labels[2]["bounds"].cpu().numpy(), ref[2]["bounds"])
    host = lsf.fusion.mesh_components((v, f, n))
    assert isinstance(host[0], np.ndarray) and _same(host[1], ref[1])


def _volume(lsf, t):
    vol = lsf.fusion.CanonicalVolume(t.shape)
    vol.tsdf.copy_(torch.from_numpy(t))
    vol.weight.fill_(1.0)
    return vol


def test_extract_mesh_removes_floaters(lsf):
    vol = _volume(lsf, S.floaters_volume())
    raw = vol.extract_mesh([0, 0, 0], 1.0, normals=True)
    assert all(_same(a, b) for a, b in zip(raw, S.floaters_mesh())) and vol.mesh_record is None
    for kw, fkw, vertices in ((dict(min_component_faces=17), dict(min_faces=17), 34 + 738 + 48),
                              (dict(keep_largest_components=1), dict(keep_largest=1), 738),
                              (dict(min_component_faces=17, keep_largest_components=2),
                               dict(min_faces=17, keep_largest=2), 738 + 48)):
        got = vol.extract_mesh([0, 0, 0], 1.0, normals=True, **kw)
        want = lsf.fusion.filter_mesh_components(raw, return_record=True, **fkw)
        assert all(_same(g, w) for g, w in zip(got, want[:3])) and vol.mesh_record == dict(components=want[3])
        assert len(got[0]) == vertices and want[3] == R.filter(*raw, None, **fkw)[4]
    # after simplify_cell: the filter sees the clustered mesh, and the record holds both
    got = vol.extract_mesh([0, 0, 0], 1.0, normals=True, simplify_cell=2.0, keep_largest_components=1)
    coarse = lsf.fusion.simplify_mesh(raw, 2.0, return_record=True)
    want = lsf.fusion.filter_mesh_components(coarse[:3], keep_largest=1, return_record=True)
    assert all(_same(g, w) for g, w in zip(got, want[:3]))
    assert vol.mesh_record == dict(coarse[3], components=want[3])
    tensors = vol.extract_mesh([0, 0, 0], 1.0, as_tensor=True, keep_largest_components=1)
    assert len(tensors) == 2 and tensors[0].is_cuda and len(tensors[0]) == 738
    plain = vol.extract_mesh([0, 0, 0], 1.0, normals=True)
    assert all(_same(a, b) for a, b in zip(plain, raw)) and vol.mesh_record is None  # the default is today's call


def test_sequence_extract_mesh_removes_floaters(lsf):
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    import moving_volume_scene as MS
    cam = DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=MS.K), depth_unit_ratio=1.0)
    seq = lsf.SequenceFusion3d(cam, (24, 24, 24), (0, 0, 0), voxel_size=1.0, narrow_band_width_voxels=3)
    seq.canonical.tsdf.copy_(torch.from_numpy(S.floaters_volume()))
    seq.canonical.weight.fill_(1.0)
    raw = seq.extract_mesh(normals=True)
    assert all(_same(a, b) for a, b in zip(raw, S.floaters_mesh()))
    assert seq.mesh_records == dict(weld=None, simplify=None)  # the default is today's call
    got = seq.extract_mesh(normals=True, min_component_faces=65, keep_largest_components=3)
    want = lsf.fusion.filter_mesh_components(raw, min_faces=65, keep_largest=3, return_record=True)
    assert all(_same(g, w) for g, w in zip(got, want[:3])) and len(got[0]) == 738 + 48
    assert seq.mesh_records == dict(weld=None, simplify=None, components=want[3])
    assert seq.canonical.mesh_record == dict(components=want[3])
    got = seq.extract_mesh(simplify_cell=2.0, keep_largest_components=1)
    coarse = lsf.fusion.simplify_mesh(raw[:2], 2.0, return_record=True)
    want = lsf.fusion.filter_mesh_components(coarse[:2], keep_largest=1, return_record=True)
    assert _same(got[0], want[0]) and _same(got[1], want[1])
    assert seq.mesh_records == dict(weld=None, simplify=coarse[2], components=want[2])


def test_refusals_that_need_the_card(D, lsf):
    v, f, n = S.floaters_mesh()
    for index in (len(v), -1):  # the two that prove the check without reaching outside the allocation without it
        faces = f.copy()
        faces[100, 2] = index
        with pytest.raises(ValueError, match="1 faces"):
            D.components(_device(v), _device(faces))
        with pytest.raises(ValueError, match="1 faces"):
            D.filter(_device(v), _device(faces), _device(n), min_faces=1)
    bad = v.copy()
    bad[17, 1] = np.nan
    with pytest.raises(ValueError, match="1 vertices"):
        D.components(_device(bad), _device(f))
    with pytest.raises(ValueError, match="1 vertices"):
        lsf.fusion.filter_mesh_components((bad, f, n), keep_largest=1)
    with pytest.raises(ValueError, match="criterion"):
        D.filter(_device(v), _device(f))
    with pytest.raises(ValueError, match="criterion"):
        lsf.fusion.filter_mesh_components((v, f, n))
    with pytest.raises(ValueError, match="3 faces"):
        D.components(_device(np.zeros((0, 3), np.float32)), _device(f[:3].copy()))  # faces without vertices


def test_empty_inputs(D):
    v, f, n = S.floaters_mesh()
    none_v, none_f = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    want = _check_components(D, none_v, none_f)
    assert want[0].shape == (0,) and want[2]["bounds"].shape == (0, 2, 3)
    assert _check_filter(D, (none_v, none_f, none_v), min_faces=1)[4]["components"] == 0
    want = _check_components(D, v, none_f)  # F = 0 with V > 0: every vertex is a component of 0 faces
    assert len(want[2]["labels"]) == len(v) and not want[2]["face_counts"].any()
    kept = _check_filter(D, (v, none_f, n), keep_largest=5)
    assert _same(kept[0], v[:5]) and kept[1].shape == (0, 3)
    assert _check_filter(D, (v, none_f, n), min_faces=1)[4]["vertices_out"] == 0
