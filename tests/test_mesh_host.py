"""CPU checks of mesh extraction: the generated case table (tools/gen_mesh_tables.py -> csrc/lsf_mesh_tables.h) and its
properties, the numpy restatement (tests/mesh_restatement.py) on analytic volumes and on the fused scene
(tests/fusion_scene.py) in world coordinates, the ctypes layout of lsf_mesh_params, the exports, the refusal of bad
arguments, the no-CPU-path error, and the PLY writer and reader."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import fusion_restatement as F
import fusion_scene as S
import mesh_restatement as M
from conftest import ROOT

G = M.G  # tools/gen_mesh_tables.py
HEADER = os.path.join(ROOT, "levelsetfusion-python_amd", "csrc", "lsf_mesh_tables.h")

# measured on a 24^3 sphere of radius 8.3 voxels (tsdf = distance / 3): the largest vertex distance from the sphere is
# 0.0147 voxel.  The bound is twice that.
SPHERE_ATOL = 0.03
# measured on the 48^3 scene, frames 0-2 fused at the true twists: the distance of a vertex from the nearest analytic
# surface is 0.109 mm on average, 1.42 mm at the 99th percentile and 4.94 mm at most (a 4 mm voxel; the largest errors
# sit on the plane's shadow edges behind the spheres).  The bounds are twice these.
SCENE_MEAN, SCENE_P99, SCENE_MAX = 2.2e-4, 2.9e-3, 9.9e-3


def _grid(shape):
    return np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")  # z, y, x


def _sphere(n, centre, radius, band=3.0):
    z, y, x = _grid((n,) * 3)
    d = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius
    return np.clip(d / band, -1, 1).astype(np.float32)


def _noise(shape, seed):
    t = np.random.default_rng(seed).uniform(-1, 1, shape).astype(np.float32)
    t[0] = t[-1] = 1
    t[:, 0] = t[:, -1] = 1
    t[:, :, 0] = t[:, :, -1] = 1
    return t


def test_the_generator_writes_the_committed_header(tmp_path):
    out = tmp_path / "tables.h"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_mesh_tables.py"), str(out)],
                          stdout=subprocess.DEVNULL)
    with open(HEADER, "rb") as f:
        assert out.read_bytes() == f.read()


def test_the_header_is_part_of_the_build_id():
    sys.path.insert(0, os.path.join(ROOT, "levelsetfusion-python_amd"))
    try:
        import _build
    finally:
        sys.path.pop(0)
    assert "lsf_mesh_tables.h" in _build.HEADERS and "lsf_mesh.hip" in _build.SOURCES


def test_case_table_properties():
    count, edges = G.tables()
    assert count[0] == 0 and count[255] == 0
    assert 1 <= count[1:255].min() and count.max() == G.MAX_TRIANGLES == 5
    for case in range(1, 255):
        crossing = {e for e in range(12) if ((case >> G.EDGE_LOW[e]) ^ (case >> G.EDGE_HIGH[e])) & 1}
        cycles = G.cycles(case)
        flat = [e for c in cycles for e in c]
        assert sorted(flat) == sorted(crossing), case  # every crossing edge in exactly one cycle
        assert [c[0] for c in cycles] == sorted(min(c) for c in cycles)
        tris = edges[case, :3 * count[case]].reshape(-1, 3)
        assert sorted(set(tris.reshape(-1).tolist())) == sorted(crossing)
        for cyc in cycles:
            if G.REVERSE:
                cyc = [cyc[0]] + cyc[1:][::-1]
            fan = G.fan(cyc)
            for k in range(2, len(fan) - 1):  # no fan diagonal joins two edges on a common cube face
                assert not G.share_face(fan[0], fan[k]), (case, fan)


@pytest.mark.parametrize("seed", range(4))
def test_padded_noise_is_a_closed_oriented_manifold(seed):
    t = _noise((14, 14, 14), seed)
    verts, faces, _ = M.extract(t, np.ones_like(t), [0, 0, 0], 1.0)
    assert len(faces) > 1000 and M.is_closed_manifold(faces)
    assert np.array_equal(np.unique(faces), np.arange(len(verts)))  # no orphan vertices


def test_sphere():
    c, r = (11.5, 11.8, 11.3), 8.3
    t = _sphere(24, c, r)
    verts, faces, normals = M.extract(t, np.ones_like(t), [0, 0, 0], 1.0, normals=True)
    assert M.is_closed_manifold(faces) and M.euler_characteristic(len(verts), faces) == 2
    dist = np.abs(np.linalg.norm(verts - np.array(c), axis=1) - r)
    assert dist.max() < SPHERE_ATOL, dist.max()
    p = verts[faces].astype(np.float64)
    face_normal = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert np.all(np.sum(face_normal * (p.mean(axis=1) - c), axis=1) > 0)  # every face points outwards
    assert np.all(np.sum(normals * (verts - np.array(c)), axis=1) > 0)
    assert np.all(np.abs(np.linalg.norm(normals, axis=1) - 1) < 1e-6)


def test_torus():
    n = 40
    z, y, x = _grid((n,) * 3)
    q = np.sqrt((x - 19.6) ** 2 + (y - 20.3) ** 2) - 11.0
    t = np.clip((np.sqrt(q ** 2 + (z - 19.8) ** 2) - 4.5) / 3, -1, 1).astype(np.float32)
    verts, faces, _ = M.extract(t, np.ones_like(t), [0, 0, 0], 1.0)
    assert M.is_closed_manifold(faces) and M.euler_characteristic(len(verts), faces) == 0


def test_a_plane_gives_an_open_mesh_bounded_by_the_volume_faces():
    shape = (16, 18, 20)
    z, y, x = _grid(shape)
    t = np.clip((0.3 * x + 0.2 * y + 0.5 * z - 9.1) / 3, -1, 1).astype(np.float32)
    verts, faces, _ = M.extract(t, np.ones_like(t), [0, 0, 0], 1.0)
    edges = M.boundary_edges(faces)
    assert len(edges) > 0 and not M.is_closed_manifold(faces)
    assert M.euler_characteristic(len(verts), faces) == 1  # a disc
    top = np.array([shape[2] - 1, shape[1] - 1, shape[0] - 1], np.float32)
    a, b = verts[edges[:, 0]], verts[edges[:, 1]]
    # both ends of every boundary edge on one face of the volume
    on_face = ((a == 0) & (b == 0)) | ((a == top) & (b == top))
    assert np.all(on_face.any(axis=1))
    d = M.directed_edges(faces)
    key = d[:, 0] * len(verts) + d[:, 1]
    assert np.unique(key).size == key.size  # oriented: no directed edge twice


def test_fused_scene_vertices_lie_on_the_analytic_surfaces():
    """frames 0-2 fused at the true twists (48^3, S.offset): the world convention agrees with fusion and ray-casting"""
    n = 48
    off = S.offset(n)
    t, w = F.empty_model((n,) * 3)
    for k, depth in enumerate(S.frames(3)):
        t, w, _ = F.fuse_depth(t, w, depth, S.K, 1.0, off, S.true_twist(k))
    verts, faces, normals = M.extract(t, w, off, normals=True)
    assert len(verts) == 3347 and len(faces) == 5804
    d = np.abs(verts[:, 2].astype(np.float64) - S.PLANE_Z)
    for c, r in S.SPHERES:
        d = np.minimum(d, np.abs(np.linalg.norm(verts - np.array(c), axis=1) - r))
    assert d.mean() < SCENE_MEAN and np.quantile(d, 0.99) < SCENE_P99 and d.max() < SCENE_MAX, \
        (d.mean(), np.quantile(d, 0.99), d.max())
    # the plane faces the camera: its normals point to -z (towards larger tsdf, the free space)
    plane = np.abs(verts[:, 2] - S.PLANE_Z) < 1e-3
    assert np.median(normals[plane, 2]) < -0.99
    # unobserved voxels (weight 0) draw nothing: an empty model has no mesh
    e = F.empty_model((n,) * 3)
    v0, f0, _ = M.extract(*e, off)
    assert v0.shape == (0, 3) and f0.shape == (0, 3)


def test_min_weight_and_iso_restrict_the_mesh():
    c, r = (11.5, 11.8, 11.3), 8.3
    t = _sphere(24, c, r)
    w = np.ones_like(t)
    w[:, :, 12:] = 0.5
    all_f = M.extract(t, w, [0, 0, 0], 1.0)[1]
    half_v, half_f, _ = M.extract(t, w, [0, 0, 0], 1.0, min_weight=0.5)
    assert 0 < len(half_f) < len(all_f) and half_v[:, 0].max() <= 12.0
    v, _, _ = M.extract(t, np.ones_like(t), [0, 0, 0], 1.0, iso=0.25)
    assert np.abs(np.linalg.norm(v - np.array(c), axis=1) - (r + 0.75)).max() < SPHERE_ATOL


def test_params_layout_and_macros():
    import levelsetfusion_python_amd._lib as lib
    p = lib.MeshParams
    assert [f[0] for f in p._fields_] == ["voxel_size", "offset_x", "offset_y", "offset_z", "iso", "min_weight",
                                          "depth", "height", "width"]
    assert ctypes.sizeof(p) == 6 * 8 + 3 * 4 + 4 and p.depth.offset == 48 and p.width.offset == 56
    header = open(os.path.join(ROOT, "include", "lsf_hip.h")).read()
    assert "#define LSF_MESH_TILE %d" % lib.MESH_TILE in header
    assert "#define LSF_MESH_MAX_TRIANGLES %d" % lib.MESH_MAX_TRIANGLES in open(HEADER).read()
    for name in ("lsf_mesh_count", "lsf_mesh_emit"):
        assert name in lib.PROTOTYPES and getattr(lib.lib, name) is not None


def _good_params():
    import levelsetfusion_python_amd._lib as lib
    p = lib.MeshParams()
    p.voxel_size, p.offset_z = 0.004, 100.0
    p.depth, p.height, p.width = 8, 8, 8
    return p


def test_the_c_abi_refuses_bad_arguments_before_launching():
    import levelsetfusion_python_amd._lib as lib
    count, emit = lib.lib.lsf_mesh_count, lib.lib.lsf_mesh_emit
    p = _good_params()
    # never dereferenced: every call below is refused on the host.  The fake buffers are 1 MiB apart, so only the
    # cases built to alias do.
    t, w, cc, em, bo, tot, vb, v, n, f = (ctypes.c_void_p((1 << 20) * k) for k in range(1, 11))
    for field, value in (("depth", 1), ("width", 0), ("height", -3), ("voxel_size", 0.0), ("voxel_size", -0.004),
                         ("voxel_size", math.nan), ("offset_y", math.inf), ("offset_x", math.nan), ("iso", math.nan),
                         ("iso", -math.inf), ("min_weight", math.nan), ("depth", 1 << 10)):
        q = lib.MeshParams.from_buffer_copy(p)
        setattr(q, field, value)
        if field == "depth" and value == 1 << 10:
            q.height = q.width = 1 << 10  # 3 * 2^30 vertices do not fit int32
        assert count(t, w, cc, em, bo, tot, ctypes.byref(q), None) == -1, (field, value)
        assert emit(t, w, cc, em, bo, vb, v, n, f, 10, 10, ctypes.byref(q), None) == -1, (field, value)
    P = ctypes.byref(p)
    assert count(None, w, cc, em, bo, tot, P, None) == -1
    assert count(t, t, cc, em, bo, tot, P, None) == -1              # tsdf is weight
    assert count(t, w, t, em, bo, tot, P, None) == -1               # cell_code aliases tsdf
    assert count(t, w, cc, cc, bo, tot, P, None) == -1              # edge_mask aliases cell_code
    assert count(t, w, cc, em, bo, None, P, None) == -1
    assert count(t, w, cc, em, bo, tot, None, None) == -1           # no params
    assert emit(t, w, cc, em, bo, vb, v, n, f, -1, 0, P, None) == -1
    assert emit(t, w, cc, em, bo, vb, v, n, f, 3 * 512 + 1, 0, P, None) == -1  # more vertices than 3 per voxel
    assert emit(t, w, cc, em, bo, vb, v, n, f, 0, 4, P, None) == -1   # faces without vertices
    assert emit(t, w, cc, em, bo, vb, None, n, f, 10, 10, P, None) == -1
    assert emit(t, w, cc, em, bo, vb, v, v, f, 10, 10, P, None) == -1  # normals alias vertices
    assert emit(t, w, cc, em, bo, vb, v, n, w, 10, 10, P, None) == -1  # faces alias weight
    near = ctypes.c_void_p((1 << 20) * 8 + 12 * 10 - 4)             # the last float of vertices
    assert emit(t, w, cc, em, bo, vb, v, near, f, 10, 10, P, None) == -1
    assert emit(t, w, cc, em, bo, vb, v, n, f, 0, 0, P, None) == 0    # nothing to emit: nothing launched


def test_host_argument_checks():
    from levelsetfusion_python_amd import device_mesh
    p = device_mesh.params((8, 9, 10), [1, 2, 3.5], 0.004, iso=0.1, min_weight=1.5)
    assert (p.depth, p.height, p.width) == (8, 9, 10) and p.offset_z == 3.5 and p.iso == 0.1 and p.min_weight == 1.5
    for bad in (dict(shape=(8, 8)), dict(shape=(1, 8, 8)), dict(shape=(1024, 1024, 1024)), dict(voxel_size=0.0),
                dict(voxel_size=math.nan), dict(voxel_size=-1.0), dict(array_offset=[0, 0]),
                dict(array_offset=[0, math.inf, 0]), dict(iso=math.nan), dict(iso=math.inf),
                dict(min_weight=math.nan)):
        kw = dict(shape=(8, 8, 8), array_offset=[0, 0, 0], voxel_size=0.004)
        kw.update(bad)
        with pytest.raises(ValueError):
            device_mesh.params(**kw)


def test_package_exports_mesh_extraction():
    import levelsetfusion_python_amd as lsf
    from levelsetfusion_python_amd import device_mesh, fusion
    assert callable(fusion.CanonicalVolume.extract_mesh) and callable(fusion.SequenceFusion3d.extract_mesh)
    assert callable(device_mesh.extract_mesh) and lsf.mesh_io is not None and "mesh_io" in lsf.__all__
    assert "extract_mesh" in fusion.__doc__ and "Mesh extraction" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_no_cpu_path():
    import torch
    from levelsetfusion_python_amd import device_mesh
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    z = torch.zeros((4, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU execution path"):
        device_mesh.extract_mesh(z, z.clone(), [0, 0, 0])


def test_ply_round_trip(tmp_path):
    from levelsetfusion_python_amd import mesh_io
    t = _sphere(16, (7.5, 7.2, 7.9), 5.1)
    verts, faces, normals = M.extract(t, np.ones_like(t), [0, 0, 0], 0.004, normals=True)
    path = str(tmp_path / "sphere.ply")
    mesh_io.write_ply(path, verts, faces, normals)
    with open(path, "rb") as f:
        data = f.read()
    head = data[:data.index(b"end_header\n") + len(b"end_header\n")].decode("ascii").split("\n")
    assert head[:2] == ["ply", "format binary_little_endian 1.0"]
    assert head[2:] == ["element vertex %d" % len(verts)] + ["property float %s" % a for a in
                                                             ("x", "y", "z", "nx", "ny", "nz")] + \
        ["element face %d" % len(faces), "property list uchar int vertex_indices", "end_header", ""]
    assert len(data) == len(b"\n".join(h.encode() for h in head)) + len(verts) * 24 + len(faces) * 13
    v, f, n = mesh_io.read_ply(path)
    assert np.array_equal(v.view(np.uint32), verts.view(np.uint32)) and np.array_equal(f, faces)
    assert np.array_equal(n.view(np.uint32), normals.view(np.uint32))
    mesh_io.write_ply(path, verts, faces)
    v, f, n = mesh_io.read_ply(path)
    assert n is None and np.array_equal(v, verts) and np.array_equal(f, faces)
    mesh_io.write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    v, f, n = mesh_io.read_ply(path)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    with pytest.raises(ValueError):
        mesh_io.write_ply(path, verts, faces + len(verts))
    with pytest.raises(ValueError):
        mesh_io.write_ply(path, verts[:, :2], faces)
