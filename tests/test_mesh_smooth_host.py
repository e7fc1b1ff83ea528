"""CPU checks of mesh smoothing: the numpy restatement (tests/mesh_smooth_restatement.py) against a plain per-vertex
Python loop, so that it is pinned independently of the kernels; that the order of the faces changes no bit; the figures
of the test sphere (Taubin keeps the volume that Laplacian passes lose); seams that stay in place; the half-sphere's
border; the header's struct and macros against the binding, the exports; the refusals of the three C entry points in a
child with every GPU hidden, and the Python refusals, which all come before a device is asked for."""
import collections
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_components_scenes as S
import mesh_restatement as M
import mesh_simplify_restatement as W
import mesh_smooth_restatement as R
import mesh_smooth_scenes as T
from conftest import ROOT


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _plain_topology(vertex_count, faces, boundary):
    count = collections.Counter()
    for face in np.asarray(faces).reshape(-1, 3).tolist():
        for a, b in ((face[0], face[1]), (face[1], face[2]), (face[2], face[0])):
            if a != b:
                count[(min(a, b), max(a, b))] += 1
    near = [set() for _ in range(vertex_count)]
    pinned = [False] * vertex_count
    for (a, b), n in count.items():
        near[a].add(b)
        near[b].add(a)
        if boundary == "fixed" and n != 2:
            pinned[a] = pinned[b] = True
    return count, near, pinned


def _plain_pass(p, near, pinned, w):
    """one pass by a loop over the vertices, in Python floats (float64, every operation rounded on its own) and ints"""
    top = max((abs(float(x)) for x in p.reshape(-1)), default=0.0)
    q = 1.0 if top == 0 else 2.0 ** (max(math.frexp(top)[1], -125) - 32)
    out = p.copy()
    for i, row in enumerate(near):
        if pinned[i] or not row:
            continue
        for a in range(3):
            total = sum(round(float(p[j, a]) / q) for j in row)  # round(): ties to even
            m = (float(total) * q) / float(len(row))
            out[i, a] = np.float32(float(p[i, a]) + w * (m - float(p[i, a])))
    return out


def _plain_smooth(v, f, iterations, lam, mu, boundary):
    count, near, pinned = _plain_topology(len(v), f, boundary)
    p = v.copy()
    for _ in range(iterations):
        p = _plain_pass(p, near, pinned, lam)
        if mu != 0:
            p = _plain_pass(p, near, pinned, mu)
    return p, count, near, pinned


def _plain_normals(v, f):
    cross = []
    for a, b, c in np.asarray(f).reshape(-1, 3).tolist():
        u = [float(v[b, k]) - float(v[a, k]) for k in range(3)]
        w = [float(v[c, k]) - float(v[a, k]) for k in range(3)]
        cross.append((u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]))
    top = max((abs(x) for c in cross for x in c), default=0.0)
    qn = 1.0 if top == 0 else 2.0 ** (math.frexp(top)[1] - 32)
    sums = [[0, 0, 0] for _ in range(len(v))]
    for face, c in zip(np.asarray(f).reshape(-1, 3).tolist(), cross):
        for corner in face:
            for k in range(3):
                sums[corner][k] += round(c[k] / qn)
    out = np.zeros((len(v), 3), np.float32)
    for i, s in enumerate(sums):
        s = [float(x) for x in s]
        length = math.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
        if length:
            out[i] = [np.float32(x / length) for x in s]
    return out


def _random_mesh(rng, vertex_count, face_count, offset=0.0, scale=2.0):
    v = (offset + rng.uniform(-scale, scale, (vertex_count, 3))).astype(np.float32)
    first = rng.integers(0, vertex_count, face_count)  # faces among near indices, some naming an index twice or thrice
    f = np.stack([first, (first + rng.integers(0, 4, face_count)) % vertex_count,
                  (first + rng.integers(0, 4, face_count)) % vertex_count], axis=1).astype(np.int32)
    return v, f


def _tetrahedron():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [5, 5, 5]], np.float32)
    return v, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int32)


@pytest.mark.parametrize("seed,vertex_count,face_count,offset,scale", [(0, 30, 40, 0.0, 2.0), (1, 120, 300, 0.0, 2.0),
                                                                       (2, 60, 20, 2.0, 0.01), (3, 7, 30, -300.0, 1.0),
                                                                       (4, 200, 150, 0.0, 1e-30)])
@pytest.mark.parametrize("boundary", ["fixed", "free"])
def test_the_restatement_equals_a_loop_over_the_vertices(seed, vertex_count, face_count, offset, scale, boundary):
    v, f = _random_mesh(np.random.default_rng(seed), vertex_count, face_count, offset, scale)
    for iterations, lam, mu in ((1, 0.5, -0.53), (3, 0.5, -0.53), (2, 1.0, 0.0), (0, 0.5, -0.53)):
        want, count, near, pinned = _plain_smooth(v, f, iterations, lam, mu, boundary)
        got = R.smooth(v, f, None, None, iterations, lam, mu, boundary)
        assert np.array_equal(_bits(got[0]), _bits(want)), (iterations, lam, mu)
        e, counts, degree, pins = R.topology(len(v), f, boundary)
        assert {tuple(k): n for k, n in zip(e.tolist(), counts.tolist())} == dict(count)
        assert degree.tolist() == [len(row) for row in near] and pins.tolist() == pinned
        assert got[4] == dict(vertices_in=vertex_count, faces_in=face_count, invalid_vertices=0, invalid_faces=0,
                              edges=len(count), boundary_edges=sum(n == 1 for n in count.values()),
                              nonmanifold_edges=sum(n > 2 for n in count.values()), pinned_vertices=sum(pinned),
                              isolated_vertices=sum(not row for row in near), max_degree=max(map(len, near)),
                              table_overflow=0, nonfinite_out=0, zero_normals=0)
    assert np.array_equal(_bits(R.vertex_normals(v, f)), _bits(_plain_normals(v, f)))


def test_small_cases_by_hand():
    v, f = _tetrahedron()
    out, _, n, _, rec = R.smooth(v, f, np.zeros_like(v), None, 1, 1.0, 0.0)
    # with lam = 1 a vertex lands on its neighbours' mean; the fifth vertex has no edge and stays
    assert np.array_equal(out, np.array([[1, 1, 1], [0, 1, 1], [1, 0, 1], [1, 1, 0], [15, 15, 15]], np.float32) / 3)
    assert rec["edges"] == 6 and rec["isolated_vertices"] == 1 and rec["pinned_vertices"] == 0
    assert rec["max_degree"] == 3 and rec["zero_normals"] == 1 and not n[4].any()
    n = R.vertex_normals(v, f)
    centre = v[:4].astype(np.float64).mean(axis=0)
    assert ((v[:4] - centre) * n[:4]).sum(axis=1).min() > 0  # the faces' right-hand normals point outwards
    assert np.allclose(np.linalg.norm(n[:4], axis=1), 1, atol=1e-6)
    # a face that names a vertex twice adds 2 to its one edge, which is then no border; one that names it thrice, nothing
    twice = np.array([[0, 0, 1], [2, 2, 2]], np.int32)
    e, counts, degree, pinned = R.topology(3, twice)
    assert e.tolist() == [[0, 1]] and counts.tolist() == [2] and degree.tolist() == [1, 1, 0] and not pinned.any()
    # an open triangle: every edge is a border, everything is pinned; free, every vertex moves to the others' mean
    tri = np.array([[0, 1, 2]], np.int32)
    assert np.array_equal(R.smooth(v[:3], tri, iterations=5)[0], v[:3])
    assert R.smooth(v[:3], tri, iterations=5)[4]["pinned_vertices"] == 3
    assert np.array_equal(R.smooth(v[:3], tri, iterations=1, lam=1.0, mu=0.0, boundary="free")[0],
                          np.array([[0.5, 0.5, 0], [0, 0.5, 0], [0.5, 0, 0]], np.float32))
    # empty meshes, and vertices without faces
    none_v, none_f = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    out = R.smooth(none_v, none_f, none_v, None, 3)
    assert out[0].shape == (0, 3) and out[2].shape == (0, 3) and out[4]["max_degree"] == 0
    out = R.smooth(v, none_f, v, None, 3)
    assert np.array_equal(out[0], v) and out[4]["isolated_vertices"] == 5 and out[4]["zero_normals"] == 5
    # the quantum: B = 3 has the exponent 2, all zeros has q = 1
    assert R.quantum(np.array([[3, -1, 0]], np.float32)) == 2.0 ** (2 - 32) and R.quantum(np.zeros((2, 3))) == 1.0
    assert R.quantum(np.array([[-4, 1, 0]], np.float32)) == 2.0 ** (3 - 32)


def test_the_order_of_the_faces_changes_no_bit():
    rng = np.random.default_rng(7)
    for mesh in (T.sphere_mesh(True), S.noise_mesh(0), T.far_mesh()):
        v, f, n = mesh
        want = R.smooth(v, f, n, None, 4)
        for _ in range(2):
            shuffled = np.roll(f[rng.permutation(len(f))], int(rng.integers(0, 3)), axis=1)  # corners rotated: same winding
            got = R.smooth(v, shuffled, n, None, 4)
            assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[2]), _bits(want[2]))
            assert got[4] == want[4]


def test_taubin_keeps_the_volume_that_laplacian_passes_lose():
    """the figures of the float32 restatement (the float64 prototype's in brackets), each against the issue's margin"""
    v, f, n = T.sphere_mesh(True)
    assert (len(v), len(f)) == (934, 1864) and M.is_closed_manifold(f)
    assert R.topology(len(v), f)[2].max() == 11
    std0, vol0 = T.radius_std(v), T.volume(v, f)
    assert abs(std0 - 0.311) < 1e-3  # 0.31100
    ten = R.smooth(v, f, n, None, 10)
    thirty = R.smooth(v, f, n, None, 30)
    plain = R.smooth(v, f, n, None, 10, mu=0.0)
    for out in (ten, thirty, plain):
        assert out[1] is not None and np.array_equal(out[1], f) and M.is_closed_manifold(out[1])
        assert out[4]["pinned_vertices"] == 0 and out[4]["boundary_edges"] == 0 and out[4]["edges"] == 2796
        assert out[4]["nonfinite_out"] == 0 and out[4]["zero_normals"] == 0
    assert T.radius_std(thirty[0]) < 0.7 * std0                    # 0.18168 (0.182): 0.584 of the input's
    assert abs(T.volume(thirty[0], f) / vol0 - 1) < 0.03           # 1.02148 (1.0215)
    assert abs(T.volume(ten[0], f) / vol0 - 1) < 0.015             # 1.00645 (1.0064)
    assert T.volume(plain[0], f) / vol0 < 0.9                      # 0.87580 (0.876)
    assert T.radius_std(ten[0]) < std0 and T.radius_std(plain[0]) < T.radius_std(ten[0])  # 0.22178, 0.12811
    cv, cf, cn = T.sphere_mesh(False)
    assert (len(cv), len(cf)) == (742, 1480)
    clean = R.smooth(cv, cf, cn, None, 10)
    assert abs(T.volume(clean[0], cf) / T.volume(cv, cf) - 1) < 0.015  # 1.00692 (1.0069)
    # the faces' winding agrees with extract_mesh's normals, "towards larger tsdf"
    dots = (R.vertex_normals(cv, cf).astype(np.float64) * cn).sum(axis=1)
    assert dots.min() > 0.95  # 0.99198
    assert ((clean[2].astype(np.float64) * cn).sum(axis=1)).min() > 0.95


def test_seams_stay_where_they_are():
    low, high, whole = S.split_noise()
    merged = S.merge([low, high])
    welded_before = W.simplify(*merged)
    assert len(welded_before[0]) == len(whole[0]) == 2820
    smooth = []
    for v, f, n in (low, high):
        e, counts, _, pinned = R.topology(len(v), f)
        out = R.smooth(v, f, n, None, 5)
        border = np.unique(e[counts == 1])
        assert len(border) and pinned[border].all()
        assert np.array_equal(_bits(out[0][pinned]), _bits(v[pinned])) and out[4]["pinned_vertices"] == pinned.sum()
        assert not np.array_equal(out[0][~pinned], v[~pinned])
        smooth.append((out[0], f, out[2]))
    welded = W.simplify(*S.merge(smooth))
    assert len(welded[0]) == len(whole[0]) and len(welded[1]) == len(whole[1])  # the seam still closes
    # free, the seam's vertices move apart and the weld no longer closes it
    loose = [R.smooth(v, f, n, None, 5, boundary="free")[:3:2] for v, f, n in (low, high)]
    apart = W.simplify(*S.merge([(a, m[1], b) for (a, b), m in zip(loose, (low, high))]))
    assert len(apart[0]) > len(whole[0])


def test_the_half_sphere_has_one_border():
    v, f, n = T.half_sphere_mesh()
    assert (len(v), len(f)) == (371, 688)
    e, counts, degree, pinned = R.topology(len(v), f)
    assert (counts == 1).sum() == 52 and (counts > 2).sum() == 0 and pinned.sum() == 52
    out = R.smooth(v, f, n, None, 10)
    assert out[4]["boundary_edges"] == 52 and out[4]["pinned_vertices"] == 52 and out[4]["nonmanifold_edges"] == 0
    assert np.array_equal(_bits(out[0][pinned]), _bits(v[pinned]))
    free = R.smooth(v, f, n, None, 10, boundary="free")
    assert free[4]["pinned_vertices"] == 0 and free[4]["boundary_edges"] == 52
    assert (free[0][pinned] != v[pinned]).any(axis=1).all()


def test_invalid_input_is_refused_by_the_restatement():
    v, f = _tetrahedron()
    for index in (5, -1):
        faces = f.copy()
        faces[1, 2] = index
        with pytest.raises(ValueError, match="1 faces"):
            R.smooth(v, faces)
        with pytest.raises(ValueError, match="1 faces"):
            R.vertex_normals(v, faces)
    for bad in (np.nan, np.inf):
        w = v.copy()
        w[1, 2] = bad
        with pytest.raises(ValueError, match="1 vertices"):
            R.smooth(w, f)
    for kw in (dict(iterations=-1), dict(iterations=1001), dict(iterations=2.5), dict(iterations=True), dict(lam=0.0),
               dict(lam=1.5), dict(lam=float("nan")), dict(mu=0.1), dict(mu=float("-inf")), dict(boundary="pinned")):
        with pytest.raises(ValueError):
            R.smooth(v, f, **kw)


def test_header_binding_and_exports():
    import levelsetfusion_python_amd as lsf
    L = lsf._lib
    header = open(os.path.join(ROOT, "include", "lsf_hip.h")).read()
    p = L.MeshSmoothParams
    assert [x[0] for x in p._fields_] == ["vertex_count", "face_count", "table_slots", "boundary_fixed", "fresh_record",
                                          "iterations", "max_blocks", "reserved", "lam", "mu"]
    assert ctypes.sizeof(p) == 8 * 4 + 2 * 8 and p.lam.offset == 32 and "} lsf_mesh_smooth_params;" in header
    for macro, value in (("TILE", L.MESH_SMOOTH_TILE), ("SCAN_THREADS", L.MESH_SMOOTH_SCAN_THREADS),
                         ("MAX_BLOCKS", L.MESH_SMOOTH_MAX_BLOCKS), ("MAX_ITERATIONS", L.MESH_SMOOTH_MAX_ITERATIONS),
                         ("VERTEX_WORDS", L.MESH_SMOOTH_VERTEX_WORDS), ("SCALAR_WORDS", L.MESH_SMOOTH_SCALAR_WORDS),
                         ("RECORD_WORDS", L.MESH_SMOOTH_RECORD_WORDS)):
        assert "#define LSF_MESH_SMOOTH_%s %d\n" % (macro, value) in header, macro
    assert "#define LSF_MESH_SMOOTH_MAX_ITEMS (1 << 27)" in header and L.MESH_SMOOTH_MAX_ITEMS == 1 << 27
    assert "#define LSF_MESH_SMOOTH_MAX_SLOTS (1 << 30)" in header and L.MESH_SMOOTH_MAX_SLOTS == 1 << 30
    assert L.MESH_SMOOTH_RECORD_FIELDS == R.RECORD_FIELDS and len(R.RECORD_FIELDS) == 13
    assert tuple(L.MESH_SMOOTH_BOUNDARIES) == R.BOUNDARIES
    assert "#define LSF_ABI_VERSION 4" in header and L.ABI_VERSION == 4 and L.lib.lsf_abi_version() == 4
    for name in ("lsf_mesh_smooth_prepare", "lsf_mesh_smooth_run", "lsf_mesh_vertex_normals"):
        assert name in L.PROTOTYPES and getattr(L.lib, name) is not None and name in header
    assert "lsf_mesh_smooth.hip" in lsf._build.SOURCES
    for name in ("smooth_mesh", "mesh_vertex_normals"):
        assert name in lsf.fusion.__all__ and callable(getattr(lsf.fusion, name)) and name in lsf.fusion.__doc__
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "Mesh smoothing" in integration and "Mesh smoothing" in lsf.fusion.__doc__ and "Mesh smoothing" in readme
    for phrase in ("cotangent weights", "feature-preserving smoothing", "a user pin mask", "smoothing the TSDF itself"):
        for text in (integration, readme, lsf.fusion.__doc__):
            assert phrase in " ".join(text.split()), phrase
    D = lsf.device_mesh_smooth
    assert [D.least_table_slots(n) for n in (0, 1, 2, 3, 5, 6, 1 << 27)] == [2, 8, 16, 32, 32, 64, 1 << 30]
    assert (D.DEFAULT_ITERATIONS, D.DEFAULT_LAM, D.DEFAULT_MU) == (10, 0.5, -0.53)
    import inspect
    for method in (lsf.fusion.CanonicalVolume.extract_mesh, lsf.fusion.SequenceFusion3d.extract_mesh):
        spec = inspect.signature(method).parameters
        assert spec["smooth_iterations"].default is None and spec["smooth_boundary"].default == "fixed"
    spec = inspect.signature(lsf.fusion.smooth_mesh).parameters
    assert [(k, x.default) for k, x in spec.items()][1:] == [
        ("iterations", 10), ("lam", 0.5), ("mu", -0.53), ("boundary", "fixed"), ("recompute_normals", True),
        ("as_tensor", False), ("return_record", False)]


# a child without torch and with every GPU hidden: the entry points' own refusals are host code, and a call that a
# refusal should have stopped must find no device to launch on
_CHILD = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
count = ctypes.c_int(-1)
hidden = lib.hipGetDeviceCount(ctypes.byref(count)) != 0 or count.value == 0
vp = ctypes.c_void_p
fns = {}
for name, pointers in (("lsf_mesh_smooth_prepare", 9), ("lsf_mesh_smooth_run", 7), ("lsf_mesh_vertex_normals", 6)):
    fns[name] = getattr(lib, name)
    fns[name].restype, fns[name].argtypes = ctypes.c_int, [vp] * (pointers + 2)
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
    """NULLs, sizes out of range, a table that is too small or no power of two, flags, iterations, lambda and mu out of
    range, misalignment, overlaps.  Made-up addresses 64 MiB apart: every refused case must return before a launch"""
    import levelsetfusion_python_amd as lsf
    L = lsf._lib
    V, F, slots = 1000, 2000, 16384
    names = dict(lsf_mesh_smooth_prepare=("vertices", "faces", "vertex_work", "edge_keys", "edge_counts", "tile_offsets",
                                          "neighbours", "scalars", "record"),
                 lsf_mesh_smooth_run=("vertices", "vertex_work", "neighbours", "out_vertices", "scratch", "scalars",
                                      "record"),
                 lsf_mesh_vertex_normals=("vertices", "faces", "sums", "normals", "scalars", "record"))
    every = dict.fromkeys(n for group in names.values() for n in group)
    base = {name: 0x10000000 + 0x4000000 * i for i, name in enumerate(every)}

    def params(**kw):
        p = L.MeshSmoothParams()
        p.vertex_count, p.face_count, p.table_slots, p.boundary_fixed, p.iterations = V, F, slots, 1, 10
        p.lam, p.mu = 0.5, -0.53
        for k, v in kw.items():
            setattr(p, k, v)
        return bytes(p).hex()

    def call(fn, passes=False, params_=None, no_params=False, **moved):
        at = dict(base, **moved)
        return dict(fn=fn, passes=passes, params=None if no_params else (params_ or params()),
                    args=[at[n] for n in names[fn]])

    refused = {}
    for fn in names:
        refused["%s without params" % fn] = call(fn, no_params=True)
        for name in names[fn]:
            refused["%s without %s" % (fn, name)] = call(fn, **{name: None})
        for field, value in (("vertex_count", -1), ("face_count", -1), ("vertex_count", (1 << 27) + 1),
                             ("face_count", (1 << 27) + 1), ("table_slots", 8192), ("table_slots", 16384 + 8),
                             ("table_slots", 12000), ("table_slots", 0), ("table_slots", -16384),
                             ("boundary_fixed", 2), ("boundary_fixed", -1), ("fresh_record", 2), ("reserved", 1),
                             ("iterations", -1), ("iterations", 1001), ("max_blocks", -1),
                             ("max_blocks", L.MESH_SMOOTH_MAX_BLOCKS + 1), ("lam", 0.0), ("lam", -0.5), ("lam", 1.25),
                             ("lam", float("nan")), ("lam", float("inf")), ("mu", 0.25), ("mu", float("nan")),
                             ("mu", float("-inf")), ("mu", float("inf"))):
            refused["%s %s %r" % (fn, field, value)] = call(fn, params_=params(**{field: value}))
    fn = "lsf_mesh_smooth_prepare"
    refused["prepare vertex_work overlaps vertices"] = call(fn, vertex_work=base["vertices"] + 12 * V - 4)
    refused["prepare record overlaps faces"] = call(fn, record=base["faces"])
    refused["prepare record off 8 bytes"] = call(fn, record=base["record"] + 4)
    refused["prepare edge_keys off 8 bytes"] = call(fn, edge_keys=base["edge_keys"] + 4)
    refused["prepare scalars off 8 bytes"] = call(fn, scalars=base["scalars"] + 4)
    refused["prepare vertices off 4 bytes"] = call(fn, vertices=base["vertices"] + 2)
    refused["prepare edge_counts overlap edge_keys"] = call(fn, edge_counts=base["edge_keys"] + 8 * slots - 4)
    refused["prepare neighbours overlap tile_offsets"] = call(fn, neighbours=base["tile_offsets"])
    refused["prepare scalars overlap record"] = call(fn, scalars=base["record"] + 8 * 12)
    fn = "lsf_mesh_smooth_run"
    refused["run out_vertices overlap vertices"] = call(fn, out_vertices=base["vertices"] + 12 * V - 4)
    refused["run scratch overlaps out_vertices"] = call(fn, scratch=base["out_vertices"])
    refused["run scratch overlaps neighbours"] = call(fn, scratch=base["neighbours"] + 4 * 6 * F - 4)
    refused["run record overlaps vertex_work"] = call(fn, record=base["vertex_work"] + 8)
    fn = "lsf_mesh_vertex_normals"
    refused["normals overlap vertices"] = call(fn, normals=base["vertices"])
    refused["normals sums overlap faces"] = call(fn, sums=base["faces"] + 12 * F - 8)
    refused["normals sums off 8 bytes"] = call(fn, sums=base["sums"] + 4)
    refused["normals overlap sums"] = call(fn, normals=base["sums"] + 24 * V - 4)
    passing = {"the plain %s" % fn: call(fn, passes=True) for fn in names}
    passing["record right behind faces"] = call("lsf_mesh_smooth_prepare", passes=True, record=base["faces"] + 12 * F)
    passing["one workgroup, free, a wide table"] = call(
        "lsf_mesh_smooth_prepare", passes=True, params_=params(max_blocks=1, boundary_fixed=0, table_slots=8 * slots))
    passing["plain passes"] = call("lsf_mesh_smooth_run", passes=True, params_=params(mu=0.0, lam=1.0, iterations=1000))
    passing["normals on their own"] = call("lsf_mesh_vertex_normals", passes=True, params_=params(fresh_record=1))
    cases = dict(refused, **passing)
    cases["normals of no vertices"] = call("lsf_mesh_vertex_normals", params_=params(vertex_count=0, face_count=0,
                                                                                     table_slots=2),
                                           vertices=None, faces=None, sums=None, normals=None)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    done = subprocess.run([sys.executable, "-c", _CHILD, L.LIB_PATH], input=json.dumps(list(cases.values())),
                          capture_output=True, text=True, env=env, timeout=120)
    assert done.returncode == 0, done.stderr
    status = dict(zip(cases, json.loads(done.stdout)))
    for name in refused:
        assert status[name] == -1, (name, status[name])
    for name in passing:  # past every check: without a device the launch itself fails; None where a device was visible
        assert status[name] is None or status[name] not in (0, -1), (name, status[name])
    assert status["normals of no vertices"] == 0  # nothing launched


def test_python_refusals_come_before_the_gpu():
    import torch
    from levelsetfusion_python_amd import device_mesh_smooth as D, fusion
    v, f = torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int32)
    n, c = torch.zeros((4, 3)), torch.zeros((4, 3), dtype=torch.uint8)
    for bad in (dict(vertices=v.double()), dict(vertices=torch.zeros((4, 2))), dict(vertices=torch.zeros(12)),
                dict(vertices=np.zeros((4, 3), np.float32)), dict(faces=f.long()),
                dict(faces=torch.zeros((2, 4), dtype=torch.int32)), dict(normals=torch.zeros((5, 3))),
                dict(normals=n.double()), dict(colours=c.int()), dict(colours=torch.zeros((4, 4), dtype=torch.uint8)),
                dict(vertices=torch.zeros((3, 4)).t()), dict(iterations=-1), dict(iterations=1001),
                dict(iterations=2.5), dict(iterations=True), dict(iterations=None), dict(iterations="3"),
                dict(lam=0.0), dict(lam=-0.1), dict(lam=1.0001), dict(lam=float("nan")), dict(lam=float("inf")),
                dict(lam=None), dict(mu=1e-9), dict(mu=float("nan")), dict(mu=float("-inf")), dict(mu="x"),
                dict(boundary="pinned"), dict(boundary=None), dict(boundary=1), dict(max_blocks=0),
                dict(max_blocks=D._lib.MESH_SMOOTH_MAX_BLOCKS + 1), dict(table_slots=8), dict(table_slots=24),
                dict(table_slots=1 << 31)):
        kw = dict(vertices=v, faces=f, normals=n, colours=c)
        kw.update(bad)
        with pytest.raises(ValueError):
            D.smooth(**kw)
    for bad in (dict(vertices=v.double()), dict(faces=f.long()), dict(max_blocks=-3)):
        with pytest.raises(ValueError):
            D.vertex_normals(**dict(dict(vertices=v, faces=f), **bad))
    with pytest.raises(ValueError, match="edge table"):
        D.params((1 << 27) + 1, 10)
    p = D.params(4, 2, 1000, 1, 0, "free")
    assert (p.iterations, p.lam, p.mu, p.boundary_fixed, p.table_slots, p.max_blocks) == (1000, 1.0, 0.0, 0, 16, 0)
    assert D.params(4, 2, np.int64(3), np.float32(0.5), -2).iterations == 3
    hv, hf = np.zeros((4, 3), np.float32), np.zeros((2, 3), np.int32)
    for mesh, kw in (((hv,), {}), ((hv, hf, hv, hv, hv), {}), ((hv.astype(np.float64), hf), {}),
                     ((hv, hf.astype(np.int64)), {}), ((hv, hf, hv, hv), {}), ((hv[:, :2], hf), {}),
                     ((hv, hf), dict(iterations=-1)), ((hv, hf), dict(iterations=1.5)), ((hv, hf), dict(lam=2.0)),
                     ((hv, hf), dict(mu=0.5)), ((hv, hf), dict(lam=float("nan"))), ((hv, hf), dict(boundary="open"))):
        with pytest.raises(ValueError):
            fusion.smooth_mesh(mesh, **kw)
    for mesh in ((hv,), (hv.astype(np.float64), hf), (hv, hf.astype(np.int64))):
        with pytest.raises(ValueError):
            fusion.mesh_vertex_normals(mesh)
    if not torch.cuda.is_available():  # past the checks there is no CPU path
        with pytest.raises(RuntimeError, match="no CPU execution path"):
            D.smooth(v, f)
        with pytest.raises(RuntimeError, match="no CPU execution path"):
            D.vertex_normals(v, f)
        with pytest.raises(RuntimeError, match="no CPU execution path"):
            fusion.smooth_mesh((hv, hf))
        with pytest.raises(RuntimeError, match="no CPU execution path"):
            fusion.mesh_vertex_normals((hv, hf, hv))
