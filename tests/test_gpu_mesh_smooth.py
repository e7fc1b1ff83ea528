"""GPU checks of mesh smoothing (csrc/lsf_mesh_smooth.hip, device_mesh_smooth, fusion.smooth_mesh and
fusion.mesh_vertex_normals) against the numpy restatement (tests/mesh_smooth_restatement.py): the bit patterns of the
positions and the normals and the whole record, exactly, at every launch shape and table size."""
import numpy as np
import pytest
import torch

import mesh_components_scenes as S
import mesh_smooth_restatement as R
import mesh_smooth_scenes as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lsf():
    import levelsetfusion_python_amd as m
    return m


@pytest.fixture(scope="module")
def D():
    from levelsetfusion_python_amd import device_mesh_smooth
    return device_mesh_smooth


def _device(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want))


def _host(out):
    return tuple(None if t is None else t.cpu().numpy() for t in out[:4]) + (out[4],)


_WANT = {}


def _want(name, mesh, **kw):
    """the restatement's result, computed once per mesh and call"""
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _WANT:
        v, f, n = mesh
        _WANT[key] = R.smooth(v, f, n, S.colours(len(v)), **kw)
    return _WANT[key]


def _check(D, name, mesh, table_slots=None, max_blocks=None, **kw):
    """smooth() with normals and colours, and without either, against the restatement; returns the restatement's"""
    v, f, n = mesh
    c = S.colours(len(v))
    want = _want(name, mesh, **kw)
    got = _host(D.smooth(_device(v), _device(f), _device(n), _device(c), return_record=True, table_slots=table_slots,
                         max_blocks=max_blocks, **kw))
    assert got[4] == want[4], (got[4], want[4])
    for g, w, what in zip(got[:4], want[:4], ("vertices", "faces", "normals", "colours")):
        assert _same(g, w), (name, what, kw)
    bare = _host(D.smooth(_device(v), _device(f), return_record=True, table_slots=table_slots, max_blocks=max_blocks,
                          **kw))
    assert bare[2] is None and bare[3] is None and bare[4] == dict(want[4], zero_normals=0)
    assert _same(bare[0], want[0]) and _same(bare[1], want[1])  # attributes change nothing else
    return want


def test_floaters_scene(D):
    mesh = S.floaters_mesh()
    assert (len(mesh[0]), len(mesh[1])) == (830, 1644)
    want = _check(D, "floaters", mesh)
    assert want[4]["edges"] == 2466 and want[4]["boundary_edges"] == 0 and want[4]["pinned_vertices"] == 0
    assert not _same(want[0], mesh[0]) and not _same(want[2], mesh[2])
    _check(D, "floaters", mesh, boundary="free")  # closed: the same answer
    assert _same(_want("floaters", mesh, boundary="free")[0], want[0])


@pytest.mark.parametrize("iterations", [1, 3, 10])
def test_noise_mesh(D, iterations):
    want = _check(D, "noise", S.noise_mesh(0), iterations=iterations)
    assert want[4]["vertices_in"] == 2820 and want[4]["nonfinite_out"] == 0


@pytest.mark.parametrize("boundary", ["fixed", "free"])
def test_half_sphere(D, boundary):
    mesh = T.half_sphere_mesh()
    want = _check(D, "half", mesh, boundary=boundary)
    assert want[4]["boundary_edges"] == 52 and want[4]["pinned_vertices"] == (52 if boundary == "fixed" else 0)
    pinned = R.topology(len(mesh[0]), mesh[1])[3]
    assert _same(want[0][pinned], mesh[0][pinned]) == (boundary == "fixed")


def test_the_calls_variants(D):
    mesh = T.sphere_mesh(True)
    plain = _check(D, "sphere", mesh, mu=0.0)
    taubin = _check(D, "sphere", mesh)
    assert abs(T.volume(taubin[0], mesh[1]) / T.volume(*mesh[:2]) - 1) < 0.015 < 0.1 < \
        1 - T.volume(plain[0], mesh[1]) / T.volume(*mesh[:2])
    none = _check(D, "sphere", mesh, iterations=0)
    assert _same(none[0], mesh[0]) and not _same(none[2], mesh[2])  # the positions as they came, the normals rebuilt
    kept = _check(D, "sphere", mesh, iterations=3, recompute_normals=False)
    assert _same(kept[2], mesh[2]) and kept[4]["zero_normals"] == 0
    _check(D, "sphere", mesh, iterations=2, lam=1.0, mu=-1.0)
    _check(D, "sphere", mesh, iterations=1, lam=0.33, mu=-0.34, boundary="free")


def test_adversarial_mesh(D):
    """a fan whose hub has a row of 8999 neighbours, a strip numbered at random, isolated vertices, degenerate faces"""
    v, f, parts = S.adversarial_mesh()
    n = np.random.default_rng(2).standard_normal(v.shape).astype(np.float32)
    want = _check(D, "adversarial", (v, f, n), iterations=2, boundary="free")
    assert want[4]["max_degree"] == 8999 and want[4]["isolated_vertices"] == parts["isolated"] + parts["thrice"]
    assert want[4]["zero_normals"] >= parts["isolated"] + parts["twice"] * 2 + parts["thrice"]
    fixed = _check(D, "adversarial", (v, f, n), iterations=2)
    assert fixed[4]["pinned_vertices"] > 0 and fixed[4]["boundary_edges"] > 0


def test_the_capped_loops_are_crossed(D):
    """more tiles of vertices, of faces and of table slots than the capped grid has workgroups, and more tile counts
    than the scan workgroup has lanes"""
    import levelsetfusion_python_amd._lib as L
    tile, max_blocks = L.MESH_SMOOTH_TILE, 64
    reach = L.MESH_SMOOTH_SCAN_THREADS * tile
    v, f, _ = S.crossing_mesh(reach)
    n = np.ascontiguousarray(v[:, ::-1])
    want = _check(D, "crossing", (v, f, n), max_blocks=max_blocks, iterations=2, boundary="free")
    one_trip = max_blocks * tile
    assert min(len(v), len(f), want[4]["edges"]) > reach > one_trip  # it crosses, the scan included
    _check(D, "crossing", (v, f, n), iterations=2, boundary="free")  # and at the library's cap of 512 workgroups
    assert len(v) > L.MESH_SMOOTH_MAX_BLOCKS * tile


def test_launch_shapes_and_table_sizes_change_nothing(D):
    mesh = S.noise_mesh(0)
    least = D.least_table_slots(len(mesh[1]))
    assert least == 65536 and 2 * 3 * len(mesh[1]) <= least < 4 * 3 * len(mesh[1])
    for max_blocks, table_slots in ((1, None), (7, least), (None, 8 * least), (1, 8 * least)):
        _check(D, "noise", mesh, iterations=3, max_blocks=max_blocks, table_slots=table_slots)
    v, f, n = T.half_sphere_mesh()
    runs = [_host(D.smooth(_device(v), _device(f), _device(n), None, return_record=True)) for _ in range(2)]
    assert all(_same(a, b) for a, b in zip(runs[0][:3], runs[1][:3])) and runs[0][4] == runs[1][4]


def test_empty_inputs(D):
    none_v, none_f = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    want = _check(D, "empty", (none_v, none_f, none_v))
    assert want[0].shape == (0, 3) and want[4]["edges"] == 0
    v, _, n = S.floaters_mesh()
    want = _check(D, "faceless", (v, none_f, n), iterations=2)  # vertices without faces: all stay, no normal
    assert _same(want[0], v) and want[4]["isolated_vertices"] == len(v) == want[4]["zero_normals"]


def test_far_from_the_origin_at_a_small_voxel(D):
    mesh = T.far_mesh()
    assert mesh[0].min() > 2.0 and np.ptp(mesh[0]) < 0.06  # B = 2 m against 4 mm edges
    want = _check(D, "far", mesh)
    assert R.quantum(mesh[0]) == 2.0 ** (2 - 32)
    near = T.sphere_mesh(True)
    moved = (want[0].astype(np.float64) - 2.0) / 0.004  # the same smoothing up to float32 rounding at 2 m
    assert np.abs(moved - _want("sphere", near)[0]).max() < 1e-3


def test_vertex_normals(D, lsf):
    for name, mesh in (("sphere", T.sphere_mesh(False)), ("noise", S.noise_mesh(0)), ("far", T.far_mesh()),
                       ("adversarial", S.adversarial_mesh()[:2])):
        v, f = mesh[:2]
        want, record = R.vertex_normals(v, f, return_record=True)
        for max_blocks in (None, 1):
            got, rec = D.vertex_normals(_device(v), _device(f), max_blocks)
            assert _same(got.cpu().numpy(), want) and rec == record, name
        assert _same(lsf.fusion.mesh_vertex_normals(mesh), want)
    v, f, n = T.sphere_mesh(False)
    got = lsf.fusion.mesh_vertex_normals((v, f))
    assert (got.astype(np.float64) * n).sum(axis=1).min() > 0.95  # towards larger tsdf, as extract_mesh's
    tensor = lsf.fusion.mesh_vertex_normals((_device(v), _device(f), _device(n)), as_tensor=True)
    assert tensor.is_cuda and _same(tensor.cpu().numpy(), got)
    coarse = lsf.fusion.simplify_mesh((v, f, n), 2.0)  # useful after simplify_mesh, which averages the normals
    assert _same(lsf.fusion.mesh_vertex_normals(coarse), R.vertex_normals(coarse[0], coarse[1]))
    empty = lsf.fusion.mesh_vertex_normals((np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)))
    assert empty.shape == (0, 3) and empty.dtype == np.float32


def test_public_function_layouts_and_tensors(lsf):
    v, f, n = S.floaters_mesh()
    c = S.colours(len(v))
    want = _want("floaters", (v, f, n))
    got = lsf.fusion.smooth_mesh((v, f, n, c), return_record=True)
    assert len(got) == 5 and all(_same(g, w) for g, w in zip(got[:4], want[:4])) and got[4] == want[4]
    assert all(isinstance(a, np.ndarray) for a in got[:4])
    got = lsf.fusion.smooth_mesh((v, f, c))
    assert len(got) == 3 and _same(got[0], want[0]) and _same(got[2], c)
    got = lsf.fusion.smooth_mesh((v, f))
    assert len(got) == 2 and _same(got[0], want[0]) and _same(got[1], f)
    tensors = lsf.fusion.smooth_mesh((_device(v), _device(f), _device(n), _device(c)), as_tensor=True)
    assert len(tensors) == 4 and all(t.is_cuda for t in tensors)
    assert all(_same(t.cpu().numpy(), w) for t, w in zip(tensors, want[:4]))
    kept = lsf.fusion.smooth_mesh((v, f, n), iterations=3, recompute_normals=False)
    assert _same(kept[2], n) and _same(kept[0], _want("floaters", (v, f, n), iterations=3)[0])
    assert _same(lsf.fusion.smooth_mesh((v, f, n), iterations=0)[0], v)


def _volume(lsf, t):
    vol = lsf.fusion.CanonicalVolume(t.shape)
    vol.tsdf.copy_(torch.from_numpy(t))
    vol.weight.fill_(1.0)
    return vol


def test_extract_mesh_smooths(lsf):
    vol = _volume(lsf, T.sphere_volume(True))
    raw = vol.extract_mesh([0, 0, 0], 1.0, normals=True)
    assert all(_same(a, b) for a, b in zip(raw, T.sphere_mesh(True))) and vol.mesh_record is None
    got = vol.extract_mesh([0, 0, 0], 1.0, normals=True, smooth_iterations=5)
    want = lsf.fusion.smooth_mesh(raw, 5, return_record=True)
    assert all(_same(g, w) for g, w in zip(got, want[:3])) and not _same(got[2], raw[2])
    assert vol.mesh_record == dict(smooth=dict(want[3], zero_normals=0, nonfinite_out=0))
    assert all(_same(g, w) for g, w in zip(got, _want("sphere", T.sphere_mesh(True), iterations=5)[:3]))
    bare = vol.extract_mesh([0, 0, 0], 1.0, smooth_iterations=5, smooth_boundary="free")
    assert len(bare) == 2 and _same(bare[0], want[0])  # closed: nothing to pin either way
    # after simplify_cell and before the component filter, and the record holds all three
    vol = _volume(lsf, S.floaters_volume())
    raw = vol.extract_mesh([0, 0, 0], 1.0, normals=True)
    got = vol.extract_mesh([0, 0, 0], 1.0, normals=True, simplify_cell=2.0, smooth_iterations=5,
                           keep_largest_components=1)
    coarse = lsf.fusion.simplify_mesh(raw, 2.0, return_record=True)
    smooth = lsf.fusion.smooth_mesh(coarse[:3], 5)
    want = lsf.fusion.filter_mesh_components(smooth, keep_largest=1, return_record=True)
    assert all(_same(g, w) for g, w in zip(got, want[:3]))
    assert set(vol.mesh_record) == set(coarse[3]) | {"smooth", "components"} and vol.mesh_record["components"] == want[3]
    tensors = vol.extract_mesh([0, 0, 0], 1.0, as_tensor=True, smooth_iterations=2)
    assert len(tensors) == 2 and tensors[0].is_cuda
    plain = vol.extract_mesh([0, 0, 0], 1.0, normals=True)
    assert all(_same(a, b) for a, b in zip(plain, raw)) and vol.mesh_record is None  # None is today's call
    for bad in (dict(smooth_iterations=-1), dict(smooth_iterations=2.5), dict(smooth_iterations=2, smooth_boundary="x")):
        with pytest.raises(ValueError):
            vol.extract_mesh([0, 0, 0], 1.0, **bad)


def test_sequence_extract_mesh_smooths(lsf):
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    import moving_volume_scene as MS
    cam = DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=MS.K), depth_unit_ratio=1.0)
    seq = lsf.SequenceFusion3d(cam, (24, 24, 24), (0, 0, 0), voxel_size=1.0, narrow_band_width_voxels=3)
    seq.canonical.tsdf.copy_(torch.from_numpy(S.floaters_volume()))
    seq.canonical.weight.fill_(1.0)
    raw = seq.extract_mesh(normals=True)
    assert all(_same(a, b) for a, b in zip(raw, S.floaters_mesh()))
    assert seq.mesh_records == dict(weld=None, simplify=None)  # None is today's call
    got = seq.extract_mesh(normals=True, smooth_iterations=5)
    want = lsf.fusion.smooth_mesh(raw, 5, return_record=True)
    assert all(_same(g, w) for g, w in zip(got, want[:3]))
    first_read = dict(want[3], zero_normals=0, nonfinite_out=0)
    assert seq.mesh_records == dict(weld=None, simplify=None, smooth=first_read)
    assert seq.canonical.mesh_record == dict(smooth=first_read)
    got = seq.extract_mesh(smooth_iterations=5, smooth_boundary="free", keep_largest_components=1)
    kept = lsf.fusion.filter_mesh_components(want[:2], keep_largest=1, return_record=True)
    assert _same(got[0], kept[0]) and _same(got[1], kept[1])
    assert seq.mesh_records == dict(weld=None, simplify=None, smooth=first_read, components=kept[2])


def test_refusals_that_need_the_card(D, lsf):
    v, f, n = S.floaters_mesh()
    for index in (len(v), -1):  # the two that prove the check without reaching outside the allocation without it
        faces = f.copy()
        faces[100, 2] = index
        with pytest.raises(ValueError, match="1 faces"):
            D.smooth(_device(v), _device(faces))
        with pytest.raises(ValueError, match="1 faces"):
            D.vertex_normals(_device(v), _device(faces))
        with pytest.raises(ValueError, match="1 faces"):
            lsf.fusion.smooth_mesh((v, faces, n))
    bad = v.copy()
    bad[17, 1] = np.nan
    bad[40, 0] = np.inf
    with pytest.raises(ValueError, match="2 vertices"):
        D.smooth(_device(bad), _device(f))
    with pytest.raises(ValueError, match="2 vertices"):
        lsf.fusion.mesh_vertex_normals((bad, f, n))
    with pytest.raises(ValueError, match="3 faces"):
        D.smooth(_device(np.zeros((0, 3), np.float32)), _device(f[:3].copy()))  # faces without vertices
    with pytest.raises(ValueError, match="3 faces"):
        D.vertex_normals(_device(np.zeros((0, 3), np.float32)), _device(f[:3].copy()))
