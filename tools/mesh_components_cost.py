"""Cost of mesh components (profiles/mesh_components_cost.md, .json) on the two meshes of tools/mesh_simplify_cost.py:
  * the mesh of tools/mesh_cost.py's 256^3 model (one synthetic depth frame fused; 46 829 vertices, one component)
  * the mesh of a padded-noise 128^3 volume (uniform noise in (-1, 1), a border of +1; 3.0 M vertices, 18 982 components)
each labelled, and filtered by keep_largest=1 and by min_faces=9, with normals, next to simplify_mesh's weld and
extract_mesh's own call on the same model in the same run:
  * the launches of each of the four foreign calls (lsf_mesh_components_label, _table, _select, _emit), each call timed
    with events on workspaces allocated once, best of 10 after a warm-up
  * the whole calls (device_mesh_components.components and .filter on device tensors) between device synchronisations,
    best of 10: what is left after the device parts is the host reads of the record, the allocations, the torch
    operations on the table and Python
  * the bytes the launches move at least once, and the rate that gives over the device time
usage: mesh_components_cost.py [OUT_STEM]      mesh_components_cost.py --trace small|large   (one call of each kind,
for rocprofv3 --kernel-trace --stats: the time of every kernel on its own)"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import mesh_cost  # noqa: E402
import mesh_simplify_cost  # noqa: E402
from levelsetfusion_python_amd import _lib, device_mesh_components as D, device_mesh_simplify  # noqa: E402
from levelsetfusion_python_amd.device_core import stream_ptr  # noqa: E402

VOXEL = mesh_simplify_cost.VOXEL
KINDS = (("keep_largest=1", dict(keep_largest=1)), ("min_faces=9", dict(min_faces=9)))


class Launches:
    """the four foreign calls of device_mesh_components.filter on workspaces and outputs allocated once"""

    def __init__(self, v, f, n, criteria):
        self.v, self.f, self.n = v, f, n
        V, F, d = len(v), len(f), v.device
        self.p = D.params(V, F, normals=True)
        tile = _lib.MESH_COMPONENTS_TILE
        self.vertex_work = torch.empty((_lib.MESH_COMPONENTS_VERTEX_WORDS, max(V, 1)), dtype=torch.int32, device=d)
        self.tiles = torch.empty(max(3 * ((V + tile - 1) // tile) + (F + tile - 1) // tile, 1), dtype=torch.int32,
                                 device=d)
        self.record = torch.empty(_lib.MESH_COMPONENTS_RECORD_WORDS, dtype=torch.int64, device=d)
        self.label()
        self.C = D.unpack_record(self.record.tolist())["components"]
        int32 = lambda count: torch.empty(count, dtype=torch.int32, device=d)  # noqa: E731
        self.labels, self.vertex_counts, self.face_counts = int32(self.C), int32(self.C), int32(self.C)
        self.bounds = torch.empty((self.C, 2, 3), dtype=torch.float32, device=d)
        self.face_labels = int32(F)
        self.table()
        table = dict(labels=self.labels, vertex_counts=self.vertex_counts, face_counts=self.face_counts,
                     bounds=self.bounds)
        self.keep = D.keep_rows(table, *D.criteria(**criteria))
        self.select()
        self.rec = D.unpack_record(self.record.tolist())
        self.out_v = torch.empty((self.rec["vertices_out"], 3), dtype=torch.float32, device=d)
        self.out_n = torch.empty((self.rec["vertices_out"], 3), dtype=torch.float32, device=d)
        self.out_f = torch.empty((self.rec["faces_out"], 3), dtype=torch.int32, device=d)
        self.workspace_bytes = sum(t.numel() * t.element_size() for t in (self.vertex_work, self.tiles))

    @staticmethod
    def _ptrs(*ts):
        return [ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None for t in ts]

    def label(self):
        _lib.check(_lib.lib.lsf_mesh_components_label(
            *self._ptrs(self.v, self.f, self.vertex_work, self.tiles, self.record), ctypes.byref(self.p), stream_ptr()),
            "lsf_mesh_components_label")

    def table(self):
        _lib.check(_lib.lib.lsf_mesh_components_table(
            *self._ptrs(self.f, self.vertex_work, self.labels, self.vertex_counts, self.face_counts, self.bounds,
                        self.face_labels), self.C, ctypes.byref(self.p), stream_ptr()), "lsf_mesh_components_table")

    def select(self):
        _lib.check(_lib.lib.lsf_mesh_components_select(
            *self._ptrs(self.f, self.vertex_work, self.keep, self.tiles, self.record), self.C, ctypes.byref(self.p),
            stream_ptr()), "lsf_mesh_components_select")

    def emit(self):
        if not self.rec["vertices_out"]:
            return
        _lib.check(_lib.lib.lsf_mesh_components_emit(
            *self._ptrs(self.v, self.f, self.n, None, self.vertex_work, self.keep, self.tiles, self.out_v, self.out_n,
                        None, self.out_f), self.C, self.rec["vertices_out"], self.rec["faces_out"],
            ctypes.byref(self.p), stream_ptr()), "lsf_mesh_components_emit")

    def moved_bytes(self):
        """bytes the launches read and write at least once, gathers and atomics counted by their words.  label: per
        vertex the position read twice (24), ten words initialised (40), parent read and label written (8), seven
        atomics at most (28), label read and row written (8); per face the indices read twice (24), two parents read
        and a compare-and-swap at least (12), a label gathered (4).  table: per vertex the row read (4), per component
        ten words read and written (80), per face an index, a label and the output (12).  select: per vertex and per
        face a label, a row and a keep word gathered (12), per face its first index (4).  emit: the same gathers again,
        per vertex the output index written (4), per output vertex position and normal read and written (48), per
        output face the indices read, three output indices gathered and the face written (36)."""
        V, F, C = len(self.v), len(self.f), self.C
        return dict(label=V * (24 + 40 + 8 + 28 + 8) + F * (24 + 12 + 4), table=V * 4 + C * 80 + F * 12,
                    select=V * 12 + F * 16,
                    emit=V * 16 + F * 16 + self.rec["vertices_out"] * 48 + self.rec["faces_out"] * 36)


def rows():
    out = []
    for name, (vol, off) in (("synthetic frame 256³", mesh_cost.model(256)),
                             ("padded noise 128³", mesh_simplify_cost.noise_model(128))):
        extract_ms = mesh_cost.best_wall_ms(lambda: vol.extract_mesh(off, VOXEL, normals=True, as_tensor=True))
        v, f, n = vol.extract_mesh(off, VOXEL, normals=True, as_tensor=True)
        weld_ms = mesh_cost.best_wall_ms(lambda: device_mesh_simplify.simplify(v, f, n, None, None))
        labels_ms = mesh_cost.best_wall_ms(lambda: D.components(v, f))
        for kind, criteria in KINDS:
            run = Launches(v, f, n, criteria)
            device = {step: mesh_cost.best_ms(getattr(run, step)) for step in ("label", "table", "select", "emit")}
            call_ms = mesh_cost.best_wall_ms(lambda: D.filter(v, f, n, None, **criteria))
            both_ms = mesh_cost.best_wall_ms(lambda: vol.extract_mesh(
                off, VOXEL, normals=True, as_tensor=True, min_component_faces=criteria.get("min_faces"),
                keep_largest_components=criteria.get("keep_largest")))
            moved = run.moved_bytes()
            total_ms = sum(device.values())
            row = dict(model=name, kind=kind, vertices_in=len(v), faces_in=len(f), components=run.C,
                       largest_component_vertices=int(run.vertex_counts.max()),
                       components_kept=run.rec["components_kept"], vertices_out=run.rec["vertices_out"],
                       faces_out=run.rec["faces_out"], workspace_bytes=run.workspace_bytes,
                       label_us=device["label"] * 1e3, table_us=device["table"] * 1e3,
                       select_us=device["select"] * 1e3, emit_us=device["emit"] * 1e3,
                       components_call_wall_us=labels_ms * 1e3, filter_call_wall_us=call_ms * 1e3,
                       filter_host_us=(call_ms - total_ms) * 1e3, weld_call_wall_us=weld_ms * 1e3,
                       extract_call_wall_us=extract_ms * 1e3, extract_with_filter_wall_us=both_ms * 1e3,
                       bytes_moved=moved, label_tb_s=moved["label"] / (device["label"] * 1e-3) / 1e12,
                       device_tb_s=sum(moved.values()) / (total_ms * 1e-3) / 1e12,
                       items_per_us=(len(v) + len(f)) / (total_ms * 1e3))
            out.append(row)
            print(json.dumps(row), flush=True)
            del run
        del vol, v, f, n
        torch.cuda.empty_cache()
    return out


# what the committed run and one traced call of each kind on the large mesh (--trace large under rocprofv3
# --kernel-trace --stats) showed
NOTES = """## Reading

One run of the tool, and one traced filter call of each kind on the large mesh (`--trace large` under
`rocprofv3 --kernel-trace --stats`) for the kernels' own times.  Nobody had measured a union-find on this chip before;
these are first figures, not a floor.

The labelling call is nearly all of the cost, and it is bound by atomics and pointer chasing, not by bandwidth: on the
large mesh its launches move the bytes counted for them at 0.19 TB/s, the four calls together at 0.37 TB/s, of the 6.3 TB/s
a copy reaches.  Per kernel, from the trace (3.0 M vertices, 6.4 M faces, 18 982 components, one of 2.9 M vertices):
`link_kernel` 1.47 ms, `face_count_kernel` 1.15 ms, `flatten_kernel` 0.55 ms, the six one-workgroup scans 0.05 ms each,
`emit_faces_kernel` 0.13 ms, `mark_faces_kernel` 0.07 ms, and `init_`, `mark_vertices_`, `face_labels_`, `table_` and
`rows_kernel` 0.02 to 0.04 ms each.  `link_kernel` is the union-find itself: per face two walks of dependent device-scope
loads and a compare-and-swap, 0.23 µs of device time per thousand faces.  `face_count_kernel` is the surprise.  It only
gathers a label per face and adds one count per wave and label, but 97 % of the faces belong to one component, so about
a hundred thousand atomic adds land on one word and serialise there at about 11 ns each; `flatten_kernel` pays the same
for its seven words per wave of that component.  Carrying the wave's largest label across the tiles a workgroup walks, so
that a word takes one atomic per wave and launch, not per wave and tile, is the next step and was not tried here.  The
filter's own launches (`select`, `emit`) move their bytes at about 1 TB/s and cost 0.43 ms together.  Labelling and
filtering 3 million vertices costs 2.6 times welding them with `simplify_mesh` (1.42 ms) and twelve times the extraction
that made them (0.31 ms).

The small mesh is one component of 46 829 vertices, and its labelling call takes 0.30 ms where seven short launches would
take about 0.05 ms: not launch-bound.  It was not traced; the supposition is `link_kernel`'s pointer chasing, since roots
are linked by index, not by rank, and a single component in voxel order can grow deep trees before path halving
flattens them.  `table`, `select` and `emit` take 0.01 to 0.02 ms each.  `filter call` is 0.39 ms with a threshold and
0.52 ms with `keep_largest` (its `argsort` and the key's arithmetic are a dozen small torch launches on a one-row
table), against 0.17 ms for welding the same mesh and 0.41 ms for extracting it; `extract_mesh` with the filter keyword
takes 0.83 to 0.96 ms.  `host` is a difference of best-of-10 figures taken in separate loops and carries their noise: on
the large mesh it comes out between -0.09 and 0.20 ms."""


def write_md(path, table, notes=None):
    notes = NOTES if notes is None else notes
    lines = ["# Cost of mesh components (MI355X)", "",
             "`tools/mesh_components_cost.py` (raw numbers: `mesh_components_cost.json`).  The two meshes of",
             "`mesh_simplify_cost.md`, both with normals: the mesh of `tools/mesh_cost.py`'s 256³ model (one synthetic",
             "depth frame fused) and the mesh of a padded-noise 128³ volume (4 mm voxels), each filtered by",
             "`keep_largest=1` and by `min_faces=9`.  `label`, `table`, `select` and `emit` are the launches of",
             "`lsf_mesh_components_label`, `_table`, `_select` and `_emit`, each call timed with events on workspaces",
             "allocated once, best of 10.  `labels call` is `device_mesh_components.components` (label, one host read,",
             "table) and `filter call` is `device_mesh_components.filter` (all four, two host reads) on device tensors",
             "between device synchronisations, best of 10; `host` = filter call - the four device parts is the two reads",
             "of the record, the allocations, the torch operations on the table and Python.  `weld` is",
             "`device_mesh_simplify.simplify` welding the same mesh and `extract` is `extract_mesh(normals=True,",
             "as_tensor=True)` on the same model, both in the same run; `both` is `extract_mesh` with the filter's",
             "keyword.  Bytes moved: what the launches read and write at least once (the tool's `moved_bytes`), gathers",
             "and atomics counted by their words, not their cache lines; `label TB/s` is the labelling call's alone.", "",
             "| mesh | kind | V in | F in | C | largest | C kept | V out | F out | label | table | select | emit "
             "| labels call | filter call | host | weld | extract | both | workspaces | bytes moved | label TB/s | TB/s "
             "| items/µs |",
             "|" + "---|" * 24]
    for r in table:
        lines.append("| %s | %s | %d | %d | %d | %d | %d | %d | %d | %.1f µs | %.1f µs | %.1f µs | %.1f µs | %.1f µs "
                     "| %.1f µs | %.1f µs | %.1f µs | %.1f µs | %.1f µs | %.1f MB | %.1f MB | %.3f | %.3f | %.1f |"
                     % (r["model"], r["kind"], r["vertices_in"], r["faces_in"], r["components"],
                        r["largest_component_vertices"], r["components_kept"], r["vertices_out"], r["faces_out"],
                        r["label_us"], r["table_us"], r["select_us"], r["emit_us"], r["components_call_wall_us"],
                        r["filter_call_wall_us"], r["filter_host_us"], r["weld_call_wall_us"],
                        r["extract_call_wall_us"], r["extract_with_filter_wall_us"], r["workspace_bytes"] / 1e6,
                        sum(r["bytes_moved"].values()) / 1e6, r["label_tb_s"], r["device_tb_s"], r["items_per_us"]))
    lines.append("")
    if notes:
        lines += [notes, ""]
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--trace":
        vol, off = mesh_cost.model(256) if sys.argv[2] == "small" else mesh_simplify_cost.noise_model(128)
        v, f, n = vol.extract_mesh(off, VOXEL, normals=True, as_tensor=True)
        sizes = [D.filter(v, f, n, None, **criteria)[4] for _, criteria in KINDS]
        torch.cuda.synchronize()
        print(json.dumps(sizes))
        return
    if len(sys.argv) > 2 and sys.argv[1] == "--md":  # the table of a run's .json written again, after NOTES changed
        with open(sys.argv[2] + ".json") as f:
            write_md(sys.argv[2] + ".md", json.load(f)["mesh_components"])
        return
    table = rows()
    stem = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mesh_components_cost")
    with open(stem + ".json", "w") as f:
        json.dump(dict(mesh_components=table), f, indent=1)
    write_md(stem + ".md", table)


if __name__ == "__main__":
    main()
