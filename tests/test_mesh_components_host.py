"""CPU checks of mesh components: the numpy restatement (tests/mesh_components_restatement.py) against a plain
breadth-first search, so that it is pinned independently of the kernels; the figures of the floaters scene and the
padded-noise mesh; the filter's ordering and ties; isolated vertices, degenerate faces and empty meshes; the header's
struct and macros against the binding, the exports, the constants that make the GPU tests' crossing shapes cross; the
refusals of the four C entry points in a child with every GPU hidden, and the Python refusals, which all come before a
device is asked for."""
import collections
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_components_restatement as R
import mesh_components_scenes as S
import mesh_restatement as M
from conftest import ROOT


def _bfs_labels(vertex_count, faces):
    """per vertex the smallest index of its component, by a breadth-first search from every vertex in index order"""
    near = collections.defaultdict(set)
    for a, b, c in np.asarray(faces).reshape(-1, 3).tolist():
        near[a].update((b, c))
        near[b].update((a, c))
        near[c].update((a, b))
    lab = [-1] * vertex_count
    for start in range(vertex_count):
        if lab[start] >= 0:
            continue
        lab[start] = start  # every smaller index is labelled already: start is its component's minimum
        queue = collections.deque([start])
        while queue:
            for w in near[queue.popleft()]:
                if lab[w] < 0:
                    lab[w] = start
                    queue.append(w)
    return np.array(lab, np.int64).reshape(-1)


def _plain_table(vertices, faces, lab):
    """the table by a loop over the components"""
    rows = []
    for l in sorted(set(lab.tolist())):
        members = vertices[lab == l].astype(np.float32) + np.float32(0.0)  # -0 + 0 is +0
        rows.append((l, int((lab == l).sum()), int((lab[faces[:, 0]] == l).sum()) if len(faces) else 0,
                     members.min(axis=0), members.max(axis=0)))
    return rows


def _same_table(table, rows):
    assert table["labels"].tolist() == [r[0] for r in rows]
    assert table["vertex_counts"].tolist() == [r[1] for r in rows]
    assert table["face_counts"].tolist() == [r[2] for r in rows]
    want = np.array([[r[3], r[4]] for r in rows], np.float32).reshape(-1, 2, 3)
    assert np.array_equal(table["bounds"].view(np.uint32), want.view(np.uint32))
    assert all(a.dtype == np.int32 for a in (table["labels"], table["vertex_counts"], table["face_counts"]))
    assert table["bounds"].dtype == np.float32 and table["bounds"].shape == (len(rows), 2, 3)


def _random_mesh(rng, vertex_count, face_count):
    v = rng.uniform(-2, 2, (vertex_count, 3)).astype(np.float32)
    v[rng.integers(0, vertex_count, 3), rng.integers(0, 3, 3)] = -0.0
    # faces among near indices, so that several components of several sizes remain, and some that repeat an index
    first = rng.integers(0, vertex_count, face_count)
    f = np.stack([first, (first + rng.integers(0, 4, face_count)) % vertex_count,
                  (first + rng.integers(0, 4, face_count)) % vertex_count], axis=1).astype(np.int32)
    return v, f


@pytest.mark.parametrize("seed,vertex_count,face_count", [(0, 40, 12), (1, 300, 90), (2, 300, 400), (3, 7, 30),
                                                          (4, 1000, 260)])
def test_the_restatement_equals_a_breadth_first_search(seed, vertex_count, face_count):
    v, f = _random_mesh(np.random.default_rng(seed), vertex_count, face_count)
    want = _bfs_labels(vertex_count, f)
    assert np.array_equal(R.labels(vertex_count, f), want)
    vertex_labels, face_labels, table = R.components(v, f)
    assert vertex_labels.dtype == np.int32 and face_labels.dtype == np.int32
    assert np.array_equal(vertex_labels, want) and np.array_equal(face_labels, want[f[:, 0]])
    _same_table(table, _plain_table(v, f, want))
    assert table["vertex_counts"].sum() == vertex_count
    assert table["face_counts"].sum() == face_count


def test_the_scenes_against_the_search_and_their_figures():
    v, f, n = S.floaters_mesh()
    assert (len(v), len(f)) == (830, 1644)
    vertex_labels, face_labels, table = R.components(v, f)
    assert np.array_equal(vertex_labels, _bfs_labels(len(v), f))
    assert tuple(table["labels"]) == S.FLOATERS_LABELS == (0, 34, 360, 782)
    assert tuple(table["vertex_counts"]) == S.FLOATERS_VERTICES == (34, 738, 10, 48)
    assert tuple(table["face_counts"]) == S.FLOATERS_FACES == (64, 1472, 16, 92)
    _same_table(table, _plain_table(v, f, vertex_labels.astype(np.int64)))
    kept = R.filter(v, f, n, None, keep_largest=1)
    assert len(kept[0]) == 738 and len(kept[1]) == 1472 and M.is_closed_manifold(kept[1])
    assert len(kept[0]) - 3 * len(kept[1]) // 2 + len(kept[1]) == 2  # Euler characteristic of a closed surface: a sphere
    assert R.filter(v, f, min_faces=64)[4]["components_kept"] == 3
    assert R.filter(v, f, min_faces=65)[4]["components_kept"] == 2
    extent = R.filter(v, f, min_extent=4.0)  # the sphere spans 12.5 voxels, the largest blob 3.2
    assert extent[4]["components_kept"] == 1 and np.array_equal(extent[1], kept[1])
    v, f, n = S.noise_mesh(0)
    vertex_labels, _, table = R.components(v, f)
    assert (len(v), len(f), len(table["labels"]), table["vertex_counts"].max()) == (2820, 5832, 29, 2608)
    assert np.array_equal(vertex_labels, _bfs_labels(len(v), f))


def test_the_adversarial_mesh_is_what_it_says():
    v, f, parts = S.adversarial_mesh()
    vertex_labels, _, table = R.components(v, f)
    assert np.array_equal(vertex_labels, _bfs_labels(len(v), f))
    assert len(table["labels"]) == sum(parts.values()) == 4203
    counts = sorted(table["vertex_counts"].tolist(), reverse=True)
    assert counts[:3] == [20000, 20000, 9000] and counts[3] == 2 and counts[-1] == 1
    assert (table["face_counts"] == 0).sum() == parts["isolated"]  # only those: a degenerate face is a face
    assert table["labels"][1] == 20000  # the reversed strip's minimum is its far end
    hub = 40000 + 9000 - 1
    assert (f == hub).any(axis=1).sum() == 9000 - 2 and vertex_labels[hub] == 40000


def test_filter_order_and_ties():
    """six components of 2, 2, 1, 1, 2 and 0 faces; the first k of (faces descending, label ascending) stay, in input order"""
    v = np.arange(16 * 3, dtype=np.float32).reshape(16, 3)
    f = np.array([[12, 13, 14], [0, 1, 2], [3, 4, 5], [1, 2, 0], [6, 7, 8], [5, 4, 3], [9, 10, 11], [14, 13, 12]],
                 np.int32)
    n = -v
    c = S.colours(16)
    table = R.components(v, f)[2]
    assert table["labels"].tolist() == [0, 3, 6, 9, 12, 15] and table["face_counts"].tolist() == [2, 2, 1, 1, 2, 0]
    order = [0, 3, 12, 6, 9, 15]
    for k in range(1, 8):
        keep = R.keep_rows(table, keep_largest=k)
        assert sorted(table["labels"][keep].tolist()) == sorted(order[:k])
    ov, of, on, oc, rec = R.filter(v, f, n, c, keep_largest=3)
    assert rec == dict(vertices_in=16, faces_in=8, invalid_vertices=0, invalid_faces=0, components=6, step_cap=0,
                       components_kept=3, vertices_out=9, faces_out=6)
    members = [0, 1, 2, 3, 4, 5, 12, 13, 14]
    assert np.array_equal(ov, v[members]) and np.array_equal(on, n[members]) and np.array_equal(oc, c[members])
    assert of.tolist() == [[6, 7, 8], [0, 1, 2], [3, 4, 5], [1, 2, 0], [5, 4, 3], [8, 7, 6]] and of.dtype == np.int32
    # thresholds first, then the k largest of what passes
    assert R.filter(v, f, min_faces=1, keep_largest=5)[4]["components_kept"] == 5
    assert R.filter(v, f, min_faces=2, keep_largest=5)[4]["components_kept"] == 3
    assert R.filter(v, f, min_vertices=3, min_faces=0)[4]["components_kept"] == 5
    assert R.filter(v, f, min_vertices=1)[4]["vertices_out"] == 16  # the isolated vertex is a component and may stay
    assert R.filter(v, f, min_faces=3)[0].shape == (0, 3)
    # an edge of exactly the threshold passes: 6 in float32 minus 0
    assert R.filter(v, f, min_extent=6.0)[4]["components_kept"] == 5
    assert R.filter(v, f, min_extent=np.nextafter(6.0, 7.0))[4]["components_kept"] == 0
    with pytest.raises(ValueError):
        R.filter(v, f)


def test_isolated_degenerate_and_empty():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, -0.0], [5, 5, 5], [6, 6, 6], [7, 7, 7]], np.float32)
    f = np.array([[4, 4, 3], [5, 5, 5], [2, 0, 2]], np.int32)
    vertex_labels, face_labels, table = R.components(v, f)
    assert vertex_labels.tolist() == [0, 1, 0, 3, 3, 5] and face_labels.tolist() == [3, 5, 0]
    assert table["labels"].tolist() == [0, 1, 3, 5] and table["vertex_counts"].tolist() == [2, 1, 2, 1]
    assert table["face_counts"].tolist() == [1, 0, 1, 1]
    assert table["bounds"][0].tolist() == [[0, 0, 0], [0, 1, 0]] and not np.signbit(table["bounds"][0]).any()
    assert table["bounds"][1].tolist() == [[1, 0, 0], [1, 0, 0]]
    none_v, none_f = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    vertex_labels, face_labels, table = R.components(none_v, none_f)
    assert vertex_labels.shape == (0,) and face_labels.shape == (0,) and table["bounds"].shape == (0, 2, 3)
    out = R.filter(none_v, none_f, min_faces=1)
    assert out[0].shape == (0, 3) and out[1].shape == (0, 3) and out[4]["components"] == 0
    vertex_labels, face_labels, table = R.components(v, none_f)  # F = 0 with V > 0: every vertex is a component
    assert vertex_labels.tolist() == list(range(6)) and face_labels.shape == (0,)
    assert table["vertex_counts"].tolist() == [1] * 6 and table["face_counts"].tolist() == [0] * 6
    out = R.filter(v, none_f, keep_largest=2)  # ties on 0 faces: the two smallest labels
    assert np.array_equal(out[0], v[:2]) and out[1].shape == (0, 3) and out[4]["components_kept"] == 2


def test_invalid_input_is_refused():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    for index in (3, -1):
        with pytest.raises(ValueError, match="1 faces"):
            R.components(v, np.array([[0, 1, 2], [0, index, 2]], np.int32))
    for bad in (np.nan, np.inf):
        w = v.copy()
        w[1, 2] = bad
        with pytest.raises(ValueError, match="1 vertices"):
            R.components(w, np.array([[0, 1, 2]], np.int32))
    with pytest.raises(ValueError, match="2 faces"):
        R.filter(np.zeros((0, 3), np.float32), np.array([[0, 1, 2], [0, 0, 0]], np.int32), min_faces=1)


def test_header_binding_exports_and_the_crossing_shapes():
    import levelsetfusion_python_amd as lsf
    L = lsf._lib
    header = open(os.path.join(ROOT, "include", "lsf_hip.h")).read()
    p = L.MeshComponentsParams
    assert [f[0] for f in p._fields_] == ["vertex_count", "face_count", "has_normals", "has_colours", "max_blocks"]
    assert ctypes.sizeof(p) == 5 * 4 and "} lsf_mesh_components_params;" in header
    for macro, value in (("TILE", L.MESH_COMPONENTS_TILE), ("SCAN_THREADS", L.MESH_COMPONENTS_SCAN_THREADS),
                         ("MAX_BLOCKS", L.MESH_COMPONENTS_MAX_BLOCKS), ("VERTEX_WORDS", L.MESH_COMPONENTS_VERTEX_WORDS),
                         ("RECORD_WORDS", L.MESH_COMPONENTS_RECORD_WORDS)):
        assert "#define LSF_MESH_COMPONENTS_%s %d\n" % (macro, value) in header, macro
    assert "#define LSF_MESH_COMPONENTS_MAX_ITEMS (1 << 29)" in header and L.MESH_COMPONENTS_MAX_ITEMS == 1 << 29
    assert L.MESH_COMPONENTS_RECORD_FIELDS == R.RECORD_FIELDS and len(R.RECORD_FIELDS) == 9
    assert lsf.device_mesh_components.TABLE_FIELDS == R.TABLE_FIELDS
    assert "#define LSF_ABI_VERSION 4" in header and L.ABI_VERSION == 4 and L.lib.lsf_abi_version() == 4
    for name in ("lsf_mesh_components_label", "lsf_mesh_components_table", "lsf_mesh_components_select",
                 "lsf_mesh_components_emit"):
        assert name in L.PROTOTYPES and getattr(L.lib, name) is not None and name in header
    assert "lsf_mesh_components.hip" in lsf._build.SOURCES
    for name in ("mesh_components", "filter_mesh_components"):
        assert name in lsf.fusion.__all__ and callable(getattr(lsf.fusion, name)) and name in lsf.fusion.__doc__
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "Mesh components" in integration and "Mesh components" in lsf.fusion.__doc__
    for phrase in ("edge-adjacency", "per-component area or volume", "components of the volume itself"):
        assert phrase in integration and phrase in lsf.fusion.__doc__.replace("\n", " ")
    # what makes tests/test_gpu_mesh_components.py's crossing mesh cross: the capped grids walk more tiles than they
    # have workgroups, and the scan workgroup more tile counts than it has lanes, for vertices, faces and components
    tile = L.MESH_COMPONENTS_TILE
    reach = max(L.MESH_COMPONENTS_MAX_BLOCKS, L.MESH_COMPONENTS_SCAN_THREADS) * tile
    assert reach == 131072
    v, f, components = S.crossing_mesh(reach)
    assert min(len(v), len(f), components) > reach
    assert min(len(v), len(f)) // tile >= max(L.MESH_COMPONENTS_MAX_BLOCKS, L.MESH_COMPONENTS_SCAN_THREADS)
    table = R.components(v, f)[2]
    assert len(table["labels"]) == components and table["face_counts"][:2].tolist() == [reach // 2 + 1] * 2
    # the adversarial mesh's parts each span many workgroups
    parts = S.adversarial_mesh()[2]
    assert min(20000, 9000, parts["isolated"], parts["twice"] + parts["thrice"]) >= 4 * tile


# a child without torch and with every GPU hidden: the entry points' own refusals are host code, and a call that a
# refusal should have stopped must find no device to launch on
_CHILD = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
count = ctypes.c_int(-1)
hidden = lib.hipGetDeviceCount(ctypes.byref(count)) != 0 or count.value == 0
vp, i64 = ctypes.c_void_p, ctypes.c_int64
types = {"label": [vp] * 7, "table": [vp] * 7 + [i64, vp, vp], "select": [vp] * 5 + [i64, vp, vp],
         "emit": [vp] * 11 + [i64] * 3 + [vp, vp]}
fns = {}
for name, argtypes in types.items():
    fns[name] = getattr(lib, "lsf_mesh_components_" + name)
    fns[name].restype, fns[name].argtypes = ctypes.c_int, argtypes
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
    """NULLs, sizes out of range, flags against their buffers, misalignment, overlaps.  Made-up addresses 16 MiB
    apart: every refused case must return before a launch"""
    import levelsetfusion_python_amd as lsf
    L = lsf._lib
    V, F, C = 1000, 2000, 40
    names = dict(label=("vertices", "faces", "vertex_work", "tile_offsets", "record"),
                 table=("faces", "vertex_work", "labels", "vertex_counts", "face_counts", "bounds", "face_labels"),
                 select=("faces", "vertex_work", "keep", "tile_offsets", "record"),
                 emit=("vertices", "faces", "normals", "colours", "vertex_work", "keep", "tile_offsets", "out_vertices",
                       "out_normals", "out_colours", "out_faces"))
    sizes = dict(label=(), table=(C,), select=(C,), emit=(C, 900, 1500))
    every = dict.fromkeys(n for group in names.values() for n in group)
    base = {name: 0x10000000 + 0x1000000 * i for i, name in enumerate(every)}

    def params(**kw):
        p = L.MeshComponentsParams()
        p.vertex_count, p.face_count, p.has_normals, p.has_colours, p.max_blocks = V, F, 1, 1, 0
        for k, v in kw.items():
            setattr(p, k, v)
        return bytes(p).hex()

    def call(fn, passes=False, params_=None, no_params=False, sizes_=None, **moved):
        at = dict(base, **moved)
        return dict(fn=fn, passes=passes, params=None if no_params else (params_ or params()),
                    args=[at[n] for n in names[fn]] + list(sizes[fn] if sizes_ is None else sizes_))

    refused = {}
    for fn in names:
        refused["%s without params" % fn] = call(fn, no_params=True)
        for name in names[fn]:
            refused["%s without %s" % (fn, name)] = call(fn, **{name: None})
        for field, value in (("vertex_count", -1), ("face_count", -1), ("vertex_count", (1 << 29) + 1),
                             ("face_count", (1 << 29) + 1), ("has_normals", -1), ("has_colours", 7), ("max_blocks", -1),
                             ("max_blocks", L.MESH_COMPONENTS_MAX_BLOCKS + 1)):
            refused["%s %s %r" % (fn, field, value)] = call(fn, params_=params(**{field: value}))
    refused["label vertex_work overlaps vertices"] = call("label", vertex_work=base["vertices"] + 12 * V - 4)
    refused["label record overlaps faces"] = call("label", record=base["faces"])
    refused["label record off 8 bytes"] = call("label", record=base["record"] + 4)
    refused["label vertices off 4 bytes"] = call("label", vertices=base["vertices"] + 2)
    refused["label tile_offsets overlap vertex_work"] = call(
        "label", tile_offsets=base["vertex_work"] + 4 * L.MESH_COMPONENTS_VERTEX_WORDS * V - 4)
    refused["table bounds overlap labels"] = call("table", bounds=base["labels"] + 4 * C - 4)
    refused["table face_labels overlap faces"] = call("table", face_labels=base["faces"] + 12 * F - 4)
    refused["select tile_offsets overlap keep"] = call("select", tile_offsets=base["keep"])
    refused["select record overlaps vertex_work"] = call("select", record=base["vertex_work"] + 8)
    refused["emit out_vertices overlap vertices"] = call("emit", out_vertices=base["vertices"] + 12 * V - 4)
    refused["emit out_faces overlap out_vertices"] = call("emit", out_faces=base["out_vertices"] + 12 * 900 - 4)
    refused["emit out_colours overlap colours"] = call("emit", out_colours=base["colours"] + 3 * V - 1)
    refused["emit out_normals without has_normals"] = call("emit", params_=params(has_normals=0))
    refused["emit colours without has_colours"] = call("emit", params_=params(has_colours=0), out_colours=None)
    for fn in ("table", "select"):
        for bad in ((-1,), (V + 1,), (0,)):
            refused["%s components %r" % (fn, bad)] = call(fn, sizes_=bad)
    for bad in ((-1, 900, 1500), (V + 1, 900, 1500), (C, -1, 0), (C, V + 1, 1500), (C, 900, F + 1), (C, 900, -1),
                (C, 0, 5)):
        refused["emit sizes %r" % (bad,)] = call("emit", sizes_=bad)
    passing = {"the plain %s" % fn: call(fn, passes=True) for fn in names}
    passing["no attributes"] = call("emit", passes=True, params_=params(has_normals=0, has_colours=0), normals=None,
                                    colours=None, out_normals=None, out_colours=None)
    passing["record right behind faces"] = call("label", passes=True, record=base["faces"] + 12 * F)
    passing["one workgroup"] = call("label", passes=True, params_=params(max_blocks=1))
    cases = dict(refused, **passing)
    cases["nothing to emit"] = call("emit", sizes_=(C, 0, 0), out_vertices=None, out_normals=None, out_colours=None,
                                    out_faces=None)
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
    from levelsetfusion_python_amd import device_mesh_components as D, fusion
    v, f = torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int32)
    n, c = torch.zeros((4, 3)), torch.zeros((4, 3), dtype=torch.uint8)
    for bad in (dict(vertices=v.double()), dict(vertices=torch.zeros((4, 2))), dict(vertices=torch.zeros(12)),
                dict(vertices=np.zeros((4, 3), np.float32)), dict(faces=f.long()),
                dict(faces=torch.zeros((2, 4), dtype=torch.int32)), dict(normals=torch.zeros((5, 3))),
                dict(normals=n.double()), dict(colours=c.int()), dict(colours=torch.zeros((4, 4), dtype=torch.uint8)),
                dict(vertices=torch.zeros((3, 4)).t()), dict(min_faces=None), dict(min_faces=-1), dict(min_faces=1.5),
                dict(min_vertices=-2), dict(min_extent=-1.0), dict(min_extent=float("nan")), dict(keep_largest=0),
                dict(keep_largest=2.5), dict(keep_largest=True), dict(max_blocks=0),
                dict(max_blocks=D._lib.MESH_COMPONENTS_MAX_BLOCKS + 1)):
        kw = dict(vertices=v, faces=f, normals=n, colours=c, min_faces=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            D.filter(**kw)
    for bad in (dict(vertices=v.double()), dict(faces=f.long()), dict(max_blocks=-3)):
        with pytest.raises(ValueError):
            D.components(**dict(dict(vertices=v, faces=f), **bad))
    with pytest.raises(ValueError, match="int32"):
        D.params((1 << 29) + 1, 10)
    assert D.criteria(min_faces=3, keep_largest=2) == (3, None, None, 2)
    assert D.criteria(min_extent=0, min_vertices=np.int64(4)) == (None, 4, 0.0, None)
    hv, hf = np.zeros((4, 3), np.float32), np.zeros((2, 3), np.int32)
    for mesh, kw in (((hv,), dict(min_faces=1)), ((hv, hf, hv, hv, hv), dict(min_faces=1)),
                     ((hv.astype(np.float64), hf), dict(min_faces=1)), ((hv, hf.astype(np.int64)), dict(min_faces=1)),
                     ((hv, hf, hv, hv), dict(min_faces=1)), ((hv[:, :2], hf), dict(min_faces=1)), ((hv, hf), {}),
                     ((hv, hf), dict(keep_largest=0)), ((hv, hf), dict(min_extent=float("inf")))):
        with pytest.raises(ValueError):
            fusion.filter_mesh_components(mesh, **kw)
    for mesh in ((hv,), (hv.astype(np.float64), hf), (hv, hf.astype(np.int64))):
        with pytest.raises(ValueError):
            fusion.mesh_components(mesh)
    # keep_rows is torch on the table alone, whatever the device: it equals the restatement's rows
    table = R.components(*S.floaters_mesh()[:2])[2]
    tensors = {k: torch.from_numpy(a) for k, a in table.items()}
    for kw in (dict(min_faces=64), dict(min_faces=65), dict(keep_largest=2), dict(min_extent=3.2, keep_largest=3),
               dict(min_vertices=11, min_faces=17), dict(keep_largest=9), dict(min_faces=5000, keep_largest=1)):
        got = D.keep_rows(tensors, **dict(dict(min_faces=None, min_vertices=None, min_extent=None, keep_largest=None),
                                          **kw))
        assert got.dtype == torch.int32 and np.array_equal(got.numpy().astype(bool), R.keep_rows(table, **kw)), kw
    if not torch.cuda.is_available():  # past the checks there is no CPU path
        with pytest.raises(RuntimeError, match="no CPU execution path"):
            D.components(v, f)
        with pytest.raises(RuntimeError, match="no CPU execution path"):
            D.filter(v, f, min_faces=1)
        with pytest.raises(RuntimeError, match="no CPU execution path"):
            fusion.mesh_components((hv, hf))
        with pytest.raises(RuntimeError, match="no CPU execution path"):
            fusion.filter_mesh_components((hv, hf), keep_largest=1)
