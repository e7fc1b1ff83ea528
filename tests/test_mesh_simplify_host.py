"""CPU checks of mesh simplification: the numpy restatement (tests/mesh_simplify_restatement.py) on the sphere and the
padded-noise volumes of the mesh tests -- the counts it gives, the invariants of its output, welding across a seam --,
the header's struct and macros against the binding, the exports, the refusals of the two C entry points in a child with
every GPU hidden, and the Python refusals, which all come before a device is asked for."""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_restatement as M
import mesh_simplify_restatement as R
from conftest import ROOT

SPHERE_CENTRE, SPHERE_RADIUS = (11.5, 11.8, 11.3), 8.3
NOISE_OFFSET, NOISE_VOXEL = (1.5, -2.0, 0.25), 0.01


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


@pytest.fixture(scope="module")
def sphere_mesh():
    t = _sphere(24, SPHERE_CENTRE, SPHERE_RADIUS)
    v, f, n = M.extract(t, np.ones_like(t), [0, 0, 0], 1.0, normals=True)
    assert len(v) == 1288 and len(f) == 2572
    return v, f, n


@pytest.fixture(scope="module")
def noise_meshes():
    out = {}
    for seed in (0, 1):
        t = _noise((14, 14, 14), seed)
        out[seed] = M.extract(t, np.ones_like(t), list(NOISE_OFFSET), NOISE_VOXEL, normals=True)
    return out


def _rows(v):
    return {tuple(r) for r in np.ascontiguousarray(v, np.float32).view(np.uint32).tolist()}


@pytest.mark.parametrize("cell,origin,vertices,faces,orphans,cancelled",
                         [(0.5, (0, 0, 0), 1135, 2266, 0, 0), (2.0, (0, 0, 0), 282, 560, 1, 1),
                          (2.5, (0.3, -0.7, 0.45), 181, 358, 0, 0), (4.0, (0.3, -0.7, 0.45), 69, 134, 2, 2),
                          (30.0, (0, 0, 0), 0, 0, 1, 0)])
def test_sphere_invariants(sphere_mesh, cell, origin, vertices, faces, orphans, cancelled):
    v, f, n = sphere_mesh
    colours = np.random.default_rng(3).integers(0, 256, (len(v), 3), dtype=np.uint8)
    ov, of, on, oc, rec = R.simplify(v, f, n, colours, cell, origin)
    assert (len(ov), len(of)) == (vertices, faces) == (rec["vertices_out"], rec["faces_out"])
    assert rec["orphan_clusters"] == orphans and rec["cancelled_groups"] == cancelled
    assert rec["clusters"] == vertices + orphans and rec["invalid_vertices"] == rec["invalid_faces"] == 0
    assert ov.shape == (vertices, 3) and of.shape == (faces, 3) and on.shape == ov.shape and oc.shape == ov.shape
    assert ov.dtype == np.float32 and of.dtype == np.int32 and on.dtype == np.float32 and oc.dtype == np.uint8
    if not vertices:
        return
    assert M.is_closed_manifold(of) and M.euler_characteristic(len(ov), of) == 2 and rec["multi_cover_groups"] == 0
    assert np.array_equal(np.unique(of), np.arange(len(ov)))  # no orphan is left
    # a representative is the mean of points within one cell: it lies under a chord of at most one cell diagonal, whose
    # sagitta is R - sqrt(R^2 - 3 cell^2 / 4), on top of the input mesh's own distance from the sphere
    centre = np.array(SPHERE_CENTRE)
    own = np.abs(np.linalg.norm(v - centre, axis=1) - SPHERE_RADIUS).max()
    bound = SPHERE_RADIUS - math.sqrt(SPHERE_RADIUS ** 2 - 3 * cell ** 2 / 4) + own
    deviation = np.abs(np.linalg.norm(ov - centre, axis=1) - SPHERE_RADIUS).max()
    assert deviation <= bound, (deviation, bound)
    assert np.all(np.abs(np.linalg.norm(on, axis=1) - 1) < 1e-6)
    assert np.all(np.sum(on * (ov - centre), axis=1) > 0)  # the summed normals still point outwards


def test_padded_noise_takes_the_other_branches(noise_meshes):
    sizes, multi, orphans = set(), {}, {}
    for seed in (0, 1):
        for cell in (0.02, 0.035):
            details = {}
            ov, of, _, _, rec = R.simplify(*noise_meshes[seed], None, cell, details=details)
            sizes |= set(details["group_sizes"].tolist())
            multi[seed, cell], orphans[seed, cell] = rec["multi_cover_groups"], rec["orphan_clusters"]
            assert rec["multi_cover_groups"] == int((np.abs(details["net"]) >= 2).sum())
            assert rec["faces_out"] == int((details["net"] != 0).sum()) == len(of)
            assert np.array_equal(np.unique(of), np.arange(len(ov)))
    assert {3, 4, 5} <= sizes
    assert multi[1, 0.035] == 6 and multi[0, 0.02] == 2
    assert all(n > 0 for n in orphans.values())
    v, f, n = noise_meshes[0]
    rec = R.simplify(v, f, n, None, 0.02)[4]
    assert (rec["vertices_in"], rec["faces_in"], rec["vertices_out"], rec["faces_out"]) == (2820, 5832, 286, 910)


def _merge(meshes):
    base, out_v, out_f = 0, [], []
    for v, f in meshes:
        out_v.append(v)
        out_f.append(f + base)
        base += len(v)
    return np.concatenate(out_v), np.concatenate(out_f).astype(np.int32)


@pytest.mark.parametrize("case,vertices,faces,chi",
                         [("sphere", 1288, 2572, 2), ("sphere at an offset", 1288, 2572, 2), ("noise", 2820, 5832, -96)])
def test_seam_weld(case, vertices, faces, chi):
    if case == "noise":
        t, off, voxel = _noise((14, 14, 14), 0), NOISE_OFFSET, NOISE_VOXEL
    else:
        t = _sphere(24, SPHERE_CENTRE, SPHERE_RADIUS)
        off, voxel = ((0, 0, 0), 1.0) if case == "sphere" else (NOISE_OFFSET, 0.004)
    w = np.ones_like(t)
    k = t.shape[2] // 2
    low = M.extract(t[:, :, :k + 1], w[:, :, :k + 1], list(off), voxel)[:2]
    high = M.extract(t[:, :, k:], w[:, :, k:], [off[0] + k, off[1], off[2]], voxel)[:2]  # as _leaving_mesh moves it
    whole_v, whole_f, _ = M.extract(t, w, list(off), voxel)
    merged = _merge([low, high])
    assert not M.is_closed_manifold(merged[1]) and len(merged[0]) > len(whole_v)
    ov, of, _, _, rec = R.simplify(*merged)
    assert (len(ov), len(of)) == (len(whole_v), len(whole_f)) == (vertices, faces)
    assert _rows(ov) == _rows(whole_v) and M.is_closed_manifold(of) and M.euler_characteristic(len(ov), of) == chi
    assert rec["degenerate_faces"] == rec["cancelled_groups"] == rec["orphan_clusters"] == 0


def test_mirror_wound_copy_welds_to_nothing_and_signed_zeros_weld(sphere_mesh):
    v, f, _ = sphere_mesh
    ov, of, _, _, rec = R.simplify(*_merge([(v, f), (v, np.ascontiguousarray(f[:, ::-1]))]))
    assert ov.shape == (0, 3) and of.shape == (0, 3) and rec["cancelled_groups"] == len(f)
    assert rec["clusters"] == rec["orphan_clusters"] == len(v)
    v2 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-0.0, 0, -0.0], [1, 1, 0]], np.float32)
    ov, of, _, _, rec = R.simplify(v2, np.array([[0, 1, 2], [3, 4, 1]], np.int32))
    assert rec["clusters"] == 4 and np.array_equal(of, [[0, 1, 2], [0, 3, 1]])
    assert np.array_equal(ov.view(np.uint32), v2[[0, 1, 2, 4]].view(np.uint32))  # the first member's bits


def test_invalid_input_is_counted():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [0, 0, 3.0e6]], np.float32)
    f = np.array([[0, 1, 2], [0, 1, 3], [0, 1, 5], [0, -1, 2], [0, 1, 4]], np.int32)
    rec = R.simplify(v, f, cell_size=2.0)[4]
    assert rec["invalid_vertices"] == 2 and rec["invalid_faces"] == 4  # the lattice ends at cell 2^20
    rec = R.simplify(v, f)[4]
    assert rec["invalid_vertices"] == 1 and rec["invalid_faces"] == 3 and rec["faces_out"] == 2


def test_header_binding_and_exports():
    import levelsetfusion_python_amd as lsf
    L = lsf._lib
    header = open(os.path.join(ROOT, "include", "lsf_hip.h")).read()
    p = L.MeshSimplifyParams
    assert [f[0] for f in p._fields_] == ["cell_size", "origin_x", "origin_y", "origin_z", "vertex_count", "face_count",
                                          "table_slots", "cluster", "has_normals", "has_colours"]
    assert ctypes.sizeof(p) == 4 * 8 + 6 * 4 and p.vertex_count.offset == 32 and p.has_colours.offset == 52
    assert "} lsf_mesh_simplify_params;" in header
    for macro, value in (("TILE", L.MESH_SIMPLIFY_TILE), ("SCAN_THREADS", L.MESH_SIMPLIFY_SCAN_THREADS),
                         ("VERTEX_WORDS", L.MESH_SIMPLIFY_VERTEX_WORDS), ("CLUSTER_WORDS", L.MESH_SIMPLIFY_CLUSTER_WORDS),
                         ("FACE_WORDS", L.MESH_SIMPLIFY_FACE_WORDS), ("RECORD_WORDS", L.MESH_SIMPLIFY_RECORD_WORDS)):
        assert "#define LSF_MESH_SIMPLIFY_%s %d\n" % (macro, value) in header, macro
    assert "#define LSF_MESH_SIMPLIFY_MAX_ITEMS (1 << 29)" in header and L.MESH_SIMPLIFY_MAX_ITEMS == 1 << 29
    assert L.MESH_SIMPLIFY_RECORD_FIELDS == R.RECORD_FIELDS and len(R.RECORD_FIELDS) == 13
    assert "#define LSF_ABI_VERSION 4" in header and L.ABI_VERSION == 4 and L.lib.lsf_abi_version() == 4
    for name in ("lsf_mesh_simplify_count", "lsf_mesh_simplify_emit"):
        assert name in L.PROTOTYPES and getattr(L.lib, name) is not None and name in header
    assert "lsf_mesh_simplify.hip" in lsf._build.SOURCES
    assert "simplify_mesh" in lsf.fusion.__all__ and callable(lsf.fusion.simplify_mesh)
    assert "Mesh simplification" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "simplify_mesh" in lsf.fusion.__doc__ and "welding vertices by position, decimation" not in lsf.fusion.__doc__


# a child without torch and with every GPU hidden: the entry points' own refusals are host code, and a call that a
# refusal should have stopped must find no device to launch on
_CHILD = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
count = ctypes.c_int(-1)
hidden = lib.hipGetDeviceCount(ctypes.byref(count)) != 0 or count.value == 0
fns = {"count": lib.lsf_mesh_simplify_count, "emit": lib.lsf_mesh_simplify_emit}
fns["count"].restype, fns["count"].argtypes = ctypes.c_int, [ctypes.c_void_p] * 13
fns["emit"].restype = ctypes.c_int
fns["emit"].argtypes = [ctypes.c_void_p] * 11 + [ctypes.c_int64] * 3 + [ctypes.c_void_p] * 2
out = []
for case in json.load(sys.stdin):
    if case["passes"] and not hidden:  # never launch on made-up pointers
        out.append(None)
        continue
    params = ctypes.create_string_buffer(bytes.fromhex(case["params"])) if case["params"] else None
    out.append(fns[case["fn"]](*case["args"], params, None))
print(json.dumps(out))
"""


def test_the_entry_points_refuse_on_their_own():
    """NULLs, sizes out of range, a table that is not a power of two or is too small, flags against their buffers,
    overlaps, a bad lattice.  Made-up addresses 16 MiB apart: every refused case must return before a launch"""
    import levelsetfusion_python_amd as lsf
    L = lsf._lib
    V, F = 1000, 2000
    count_names = ("vertices", "faces", "normals", "colours", "table", "vertex_work", "cluster_work", "sums",
                   "face_work", "tile_offsets", "record")
    emit_names = ("vertices", "faces", "vertex_work", "cluster_work", "sums", "face_work", "tile_offsets",
                  "out_vertices", "out_normals", "out_colours", "out_faces")
    base = {name: 0x10000000 + 0x1000000 * i for i, name in enumerate(dict.fromkeys(count_names + emit_names))}

    def params(**kw):
        p = L.MeshSimplifyParams()
        p.cell_size, p.vertex_count, p.face_count, p.table_slots = 2.0, V, F, 4096
        p.cluster, p.has_normals, p.has_colours = 1, 1, 1
        for k, v in kw.items():
            setattr(p, k, v)
        return bytes(p).hex()

    def count(passes=False, params_=None, no_params=False, **moved):
        at = dict(base, **moved)
        return dict(fn="count", passes=passes, params=None if no_params else (params_ or params()),
                    args=[at[n] for n in count_names])

    def emit(passes=False, params_=None, sizes=(900, 800, 1500), **moved):
        at = dict(base, **moved)
        return dict(fn="emit", passes=passes, params=params_ or params(), args=[at[n] for n in emit_names] + list(sizes))

    refused = {"no params": count(no_params=True)}
    for name in count_names:
        refused["count without %s" % name] = count(**{name: None})
    for name in emit_names:
        refused["emit without %s" % name] = emit(**{name: None})
    for field, value in (("vertex_count", -1), ("face_count", -1), ("vertex_count", (1 << 29) + 1),
                         ("table_slots", 4095), ("table_slots", 3000), ("table_slots", 2048), ("table_slots", 0),
                         ("table_slots", -4096), ("cluster", 2), ("has_normals", -1), ("has_colours", 7),
                         ("cell_size", 0.0), ("cell_size", -2.0), ("cell_size", math.nan), ("cell_size", math.inf),
                         ("origin_x", math.nan), ("origin_z", math.inf)):
        refused["count %s %r" % (field, value)] = count(params_=params(**{field: value}))
        refused["emit %s %r" % (field, value)] = emit(params_=params(**{field: value}))
    refused["normals without has_normals"] = count(params_=params(has_normals=0))
    refused["has_colours without colours"] = count(colours=None)
    refused["table overlaps vertices"] = count(table=base["vertices"] + 12 * V - 4)
    refused["record overlaps faces"] = count(record=base["faces"])
    refused["sums overlap vertex_work"] = count(sums=base["vertex_work"] + 20 * V - 8)
    refused["tile_offsets overlap face_work"] = count(tile_offsets=base["face_work"] + 28 * F - 4)
    refused["out_vertices overlap vertices"] = emit(out_vertices=base["vertices"] + 12 * V - 4)
    refused["out_faces overlap out_vertices"] = emit(out_faces=base["out_vertices"] + 12 * 800 - 4)
    refused["out_normals without has_normals"] = emit(params_=params(has_normals=0))
    for sizes in ((-1, 0, 0), (V + 1, 800, 1500), (900, 901, 1500), (900, 800, F + 1), (900, 800, -1), (900, 0, 5)):
        refused["emit sizes %r" % (sizes,)] = emit(sizes=sizes)
    passing = {"the plain count": count(passes=True),
               "weld reads no lattice": count(passes=True, params_=params(cluster=0, cell_size=math.nan)),
               "no attributes": count(passes=True, params_=params(cluster=0, has_normals=0, has_colours=0),
                                      normals=None, colours=None, sums=None),
               "record right behind faces": count(passes=True, record=base["faces"] + 12 * F),
               "the plain emit": emit(passes=True)}
    cases = dict(refused, **passing)
    nothing = emit(sizes=(900, 0, 0), out_vertices=None, out_normals=None, out_colours=None, out_faces=None)
    cases["nothing to emit"] = nothing
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    done = subprocess.run([sys.executable, "-c", _CHILD, L.LIB_PATH], input=json.dumps(list(cases.values())),
                          capture_output=True, text=True, env=env, timeout=120)
    assert done.returncode == 0, done.stderr
    status = dict(zip(cases, json.loads(done.stdout)))
    for name in refused:
        assert status[name] == -1, (name, status[name])
    for name in passing:  # past every check: without a device the launch itself fails; None where a device was visible
        assert status[name] is None or status[name] not in (0, -1), (name, status[name])
    assert status["nothing to emit"] == 0  # nothing launched


def test_python_refusals_come_before_the_gpu():
    import torch
    from levelsetfusion_python_amd import device_mesh_simplify as D, fusion
    v, f = torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int32)
    n, c = torch.zeros((4, 3)), torch.zeros((4, 3), dtype=torch.uint8)
    for bad in (dict(vertices=v.double()), dict(vertices=torch.zeros((4, 2))), dict(vertices=torch.zeros(12)),
                dict(vertices=np.zeros((4, 3), np.float32)), dict(faces=f.long()),
                dict(faces=torch.zeros((2, 4), dtype=torch.int32)),
                dict(normals=torch.zeros((5, 3))), dict(normals=n.double()), dict(colours=c.int()),
                dict(colours=torch.zeros((4, 4), dtype=torch.uint8)), dict(vertices=torch.zeros((3, 4)).t()),
                dict(cell_size=0.0), dict(cell_size=-1.0), dict(cell_size=math.nan), dict(cell_size=math.inf),
                dict(origin=(0, 0)), dict(origin=(0, math.nan, 0)), dict(origin=(math.inf, 0, 0)),
                dict(table_slots=6), dict(table_slots=4), dict(table_slots=1 << 31)):
        kw = dict(vertices=v, faces=f, normals=n, colours=c, cell_size=1.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            D.simplify(**kw)
    assert D.smallest_table_slots(4, 2) == 8 and D.smallest_table_slots(0, 0) == 2 and D.smallest_table_slots(5, 9) == 32
    with pytest.raises(ValueError, match="int32"):
        D.params((1 << 29) + 1, 10)
    hv, hf = np.zeros((4, 3), np.float32), np.zeros((2, 3), np.int32)
    for mesh, kw in (((hv,), {}), ((hv, hf, hv, hv, hv), {}), ((hv.astype(np.float64), hf), {}),
                     ((hv, hf.astype(np.int64)), {}), ((hv, hf, hv, hv), {}), ((hv[:, :2], hf), {}),
                     ((hv, hf), dict(cell_size=0.0)), ((hv, hf), dict(cell_size=math.nan)),
                     ((hv, hf), dict(origin=(0, math.inf, 0)))):
        with pytest.raises(ValueError):
            fusion.simplify_mesh(mesh, **kw)
    if not torch.cuda.is_available():  # past the checks there is no CPU path
        with pytest.raises(RuntimeError, match="no CPU execution path"):
            D.simplify(v, f)
        with pytest.raises(RuntimeError, match="no CPU execution path"):
            fusion.simplify_mesh((hv, hf))
        with pytest.raises(RuntimeError, match="no CPU execution path"):
            fusion.merge_meshes([(hv, hf), (hv, hf)], weld=True)
    merged = fusion.merge_meshes([(hv, hf), (hv, hf)])
    assert len(merged[0]) == 8 and len(merged[1]) == 4  # the default is today's concatenation
