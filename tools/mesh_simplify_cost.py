"""Cost of mesh simplification (profiles/mesh_simplify_cost.md, .json) on two meshes:
  * the mesh of tools/mesh_cost.py's 256^3 model (one synthetic depth frame fused; 46 829 vertices): launch-bound
  * the mesh of a padded-noise 128^3 volume (uniform noise in (-1, 1), a border of +1; millions of vertices): throughput
each welded and clustered at cells of 2 and 4 voxels, with normals, next to extract_mesh's own call on the same model
in the same run:
  * the counting launches (lsf_mesh_simplify_count) and the emitting launches (lsf_mesh_simplify_emit), each timed with
    events on workspaces allocated once, best of 10 after a warm-up
  * the whole call (device_mesh_simplify.simplify on device tensors) between device synchronisations, best of 10: what
    is left after the two device parts is the host read of the record, the allocations and Python
  * the bytes the launches move at least once, and the rate that gives over the device time
usage: mesh_simplify_cost.py [OUT_STEM]      mesh_simplify_cost.py --trace small|large   (one call of each kind, for
rocprofv3 --kernel-trace --stats)"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import levelsetfusion_python_amd as lsf  # noqa: E402
import mesh_cost  # noqa: E402
from levelsetfusion_python_amd import _lib, device_mesh_simplify as D  # noqa: E402
from levelsetfusion_python_amd.device_core import stream_ptr  # noqa: E402

VOXEL = 0.004
KINDS = (("weld", None), ("cluster 2 voxels", 2 * VOXEL), ("cluster 4 voxels", 4 * VOXEL))


def noise_model(n, seed=0):
    t = np.random.default_rng(seed).uniform(-1, 1, (n, n, n)).astype(np.float32)
    t[0] = t[-1] = 1
    t[:, 0] = t[:, -1] = 1
    t[:, :, 0] = t[:, :, -1] = 1
    vol = lsf.fusion.CanonicalVolume(n)
    vol.tsdf.copy_(torch.from_numpy(t))
    vol.weight.fill_(1.0)
    torch.cuda.synchronize()
    return vol, np.zeros(3)


class Launches:
    """the two halves of device_mesh_simplify.simplify on workspaces and outputs allocated once"""

    def __init__(self, v, f, n, cell):
        self.v, self.f, self.n = v, f, n
        V, F = len(v), len(f)
        self.p = D.params(V, F, cell, normals=True)
        d = v.device
        k = 3 * (self.p.cluster + 1)
        tile = _lib.MESH_SIMPLIFY_TILE
        int32 = lambda words: torch.empty(max(words, 1), dtype=torch.int32, device=d)  # noqa: E731
        self.table = int32(self.p.table_slots)
        self.vertex_work = int32(_lib.MESH_SIMPLIFY_VERTEX_WORDS * V)
        self.cluster_work = int32(_lib.MESH_SIMPLIFY_CLUSTER_WORDS * V)
        self.sums = torch.empty(k * V, dtype=torch.int64, device=d)
        self.face_work = int32(_lib.MESH_SIMPLIFY_FACE_WORDS * F)
        self.tiles = int32(3 * ((V + tile - 1) // tile) + 3 * ((F + tile - 1) // tile))
        self.record = torch.empty(_lib.MESH_SIMPLIFY_RECORD_WORDS, dtype=torch.int64, device=d)
        self.count()
        self.rec = D.unpack_record(self.record.tolist())
        self.out_v = torch.empty((self.rec["vertices_out"], 3), dtype=torch.float32, device=d)
        self.out_n = torch.empty((self.rec["vertices_out"], 3), dtype=torch.float32, device=d)
        self.out_f = torch.empty((self.rec["faces_out"], 3), dtype=torch.int32, device=d)
        self.workspace_bytes = sum(t.numel() * t.element_size() for t in (
            self.table, self.vertex_work, self.cluster_work, self.sums, self.face_work, self.tiles))

    @staticmethod
    def _ptrs(*ts):
        return [ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None for t in ts]

    def count(self):
        _lib.check(_lib.lib.lsf_mesh_simplify_count(
            *self._ptrs(self.v, self.f, self.n, None, self.table, self.vertex_work, self.cluster_work, self.sums,
                        self.face_work, self.tiles, self.record), ctypes.byref(self.p), stream_ptr()),
            "lsf_mesh_simplify_count")

    def emit(self):
        _lib.check(_lib.lib.lsf_mesh_simplify_emit(
            *self._ptrs(self.v, self.f, self.vertex_work, self.cluster_work, self.sums, self.face_work, self.tiles,
                        self.out_v, self.out_n, None, self.out_f), self.rec["clusters"], self.rec["vertices_out"],
            self.rec["faces_out"], ctypes.byref(self.p), stream_ptr()), "lsf_mesh_simplify_emit")

    def moved_bytes(self):
        """bytes the launches read and write at least once.  Per vertex: position 12 and normal 12 read; key 12, slot 4
        (twice: the validity, then the slot) and cluster id 4 written, key 12, slot 3 x 4 and id 4 read; members,
        used and first 12 cleared or written; the sums' row cleared (8 K) and one 8-byte atomic per word.  Per table
        slot: 4 cleared twice and a 4-byte atomic per item.  Per face: indices 12 read twice, three ids gathered twice
        (24), key 12 written and read twice (36), state 4 written three times and read three times (24), net and the
        two minima cleared (12) and hit by three atomics (12).  Per output vertex 24 and per output face 12 written."""
        V, F, k = len(self.v), len(self.f), 3 * (self.p.cluster + 1)
        return (V * (24 + 12 + 8 + 4 + 12 + 12 + 4 + 12 + 16 * k) + self.p.table_slots * 8 + (V + F) * 4
                + F * (24 + 24 + 12 + 36 + 24 + 12 + 12) + self.rec["vertices_out"] * 24 + self.rec["faces_out"] * 12)


def rows():
    out = []
    for name, (vol, off) in (("synthetic frame 256³", mesh_cost.model(256)), ("padded noise 128³", noise_model(128))):
        extract_ms = mesh_cost.best_wall_ms(lambda: vol.extract_mesh(off, VOXEL, normals=True, as_tensor=True))
        v, f, n = vol.extract_mesh(off, VOXEL, normals=True, as_tensor=True)
        for kind, cell in KINDS:
            run = Launches(v, f, n, cell)
            count_ms = mesh_cost.best_ms(run.count)
            emit_ms = mesh_cost.best_ms(run.emit)
            call_ms = mesh_cost.best_wall_ms(lambda: D.simplify(v, f, n, None, cell))
            both_ms = mesh_cost.best_wall_ms(lambda: vol.extract_mesh(off, VOXEL, normals=True, as_tensor=True,
                                                                      simplify_cell=cell)) if cell else None
            moved = run.moved_bytes()
            row = dict(model=name, kind=kind, vertices_in=len(v), faces_in=len(f), vertices_out=run.rec["vertices_out"],
                       faces_out=run.rec["faces_out"], clusters=run.rec["clusters"],
                       degenerate_faces=run.rec["degenerate_faces"], cancelled_groups=run.rec["cancelled_groups"],
                       multi_cover_groups=run.rec["multi_cover_groups"], table_slots=run.p.table_slots,
                       workspace_bytes=run.workspace_bytes, count_us=count_ms * 1e3, emit_us=emit_ms * 1e3,
                       call_wall_us=call_ms * 1e3, host_us=(call_ms - count_ms - emit_ms) * 1e3,
                       extract_call_wall_us=extract_ms * 1e3,
                       extract_with_simplify_cell_wall_us=None if both_ms is None else both_ms * 1e3,
                       bytes_moved=moved, device_tb_s=moved / ((count_ms + emit_ms) * 1e-3) / 1e12,
                       items_per_us=(len(v) + len(f)) / ((count_ms + emit_ms) * 1e3))
            out.append(row)
            print(json.dumps(row), flush=True)
            del run
        del vol, v, f, n
        torch.cuda.empty_cache()
    return out


# what one traced call of each kind on the large mesh (--trace large under rocprofv3 --kernel-trace --stats) showed when the
# committed table was measured
NOTES = """## Reading

The small mesh is launch-bound: about twenty short launches and fills take about 100 µs of device time for 140 thousand
items, the same whatever the kind, and a third of the call is the host (the record's read, eight allocations, Python).
A call costs about 0.4 of `extract_mesh`'s own on that model.

The large mesh is bound by atomics, not by bandwidth: the launches move their bytes at about 1 TB/s of the 6.3 TB/s a
copy reaches.  Per kernel, from the trace: clustering spends 0.84 to 0.95 ms of its 1.7 ms in the accumulate launch,
whose seven 64-bit integer atomic adds per vertex (the member count, three q, three m) land on the few words of each
cluster's row -- 12 members per cluster at 2 voxels, 92 at 4 -- and serialise there; the vertex insert launch
(compare-and-swap and probing in a 64 MB table) takes 0.24 to 0.29 ms.  Welding has one member per cluster, so its
accumulate launch takes 0.18 ms, and its largest launches are the two inserts, 0.24 ms for the vertices and 0.42 ms for
6.4 million distinct face triples: random 4-byte atomics over the 64 MB table, bound by the atomic rate of the L2 and
the memory side behind it.  The one-workgroup scans take 0.03 to 0.15 ms each at 12 to 25 thousand tiles.  Every tile
adding its statistics to the record with an atomic of its own cost 0.3 to 0.5 ms per such launch (25 thousand atomics
on one address) before the scans took those sums over.  On this mesh `extract_mesh` itself takes 0.31 ms: simplifying
3 million vertices and 6.4 million faces costs five times the extraction that made them."""


def write_md(path, table, notes=NOTES):
    lines = ["# Cost of mesh simplification (MI355X)", "",
             "`tools/mesh_simplify_cost.py` (raw numbers: `mesh_simplify_cost.json`).  Two meshes, both with normals:",
             "the mesh of `tools/mesh_cost.py`'s 256³ model (one synthetic depth frame fused) and the mesh of a",
             "padded-noise 128³ volume, each welded and clustered at cells of 2 and 4 voxels (4 mm voxels).  `count` is",
             "the launches of `lsf_mesh_simplify_count` and `emit` those of `lsf_mesh_simplify_emit`, each timed with",
             "events on workspaces allocated once, best of 10.  `call` is `device_mesh_simplify.simplify` on device",
             "tensors between device synchronisations, best of 10; `host` = call - count - emit is the read of the",
             "record, the allocation of the workspaces and outputs, and Python.  `extract` is",
             "`extract_mesh(normals=True, as_tensor=True)` on the same model in the same run, `both` the same call with",
             "`simplify_cell=`.  Bytes moved: what the launches read and write at least once (the tool's",
             "`moved_bytes`), gathers and atomics counted by their words, not their cache lines.", "",
             "| mesh | kind | V in | F in | V out | F out | count | emit | call | host | extract | both | workspaces "
             "| bytes moved | TB/s | items/µs |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in table:
        both = "—" if r["extract_with_simplify_cell_wall_us"] is None else "%.1f µs" % r["extract_with_simplify_cell_wall_us"]
        lines.append("| %s | %s | %d | %d | %d | %d | %.1f µs | %.1f µs | %.1f µs | %.1f µs | %.1f µs | %s | %.1f MB "
                     "| %.1f MB | %.3f | %.1f |"
                     % (r["model"], r["kind"], r["vertices_in"], r["faces_in"], r["vertices_out"], r["faces_out"],
                        r["count_us"], r["emit_us"], r["call_wall_us"], r["host_us"], r["extract_call_wall_us"], both,
                        r["workspace_bytes"] / 1e6, r["bytes_moved"] / 1e6, r["device_tb_s"], r["items_per_us"]))
    lines.append("")
    if notes:
        lines += [notes, ""]
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--trace":
        vol, off = mesh_cost.model(256) if sys.argv[2] == "small" else noise_model(128)
        v, f, n = vol.extract_mesh(off, VOXEL, normals=True, as_tensor=True)
        sizes = [D.simplify(v, f, n, None, cell)[4] for _, cell in KINDS]
        torch.cuda.synchronize()
        print(json.dumps(sizes))
        return
    table = rows()
    stem = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mesh_simplify_cost")
    with open(stem + ".json", "w") as f:
        json.dump(dict(mesh_simplify=table), f, indent=1)
    write_md(stem + ".md", table)


if __name__ == "__main__":
    main()
