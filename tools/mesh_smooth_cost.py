"""Cost of mesh smoothing (profiles/mesh_smooth_cost.md, .json) on the two meshes of tools/mesh_simplify_cost.py:
  * the mesh of tools/mesh_cost.py's 256^3 model (one synthetic depth frame fused; 46 829 vertices, an open sheet)
  * the mesh of a padded-noise 128^3 volume (uniform noise in (-1, 1), a border of +1; 3.0 M vertices, closed)
each smoothed by the default 10 Taubin iterations (20 passes) with normals, next to simplify_mesh's weld,
filter_mesh_components(keep_largest=1) and extract_mesh's own call on the same model in the same run:
  * the launches of each of the three foreign calls (lsf_mesh_smooth_prepare, _run, lsf_mesh_vertex_normals), each call
    timed with events on workspaces allocated once, best of 10 after a warm-up; a pass is the run's time by its passes
  * the whole call (device_mesh_smooth.smooth on device tensors) between device synchronisations, best of 10: what is
    left after the device parts is the host read of the record, the allocations and Python
  * the bytes a pass moves at least once, and the rate that gives over a pass's device time
  * a lambda | mu pass pair written with torch.index_add_ on the same edge list (float32 sums by float atomics, so not
    the same bits from run to run), timed with events: what the HIP path buys
  * the figures of the 24^3 test sphere (tests/mesh_smooth_scenes.py) that tests/test_mesh_smooth_host.py asserts on the
    restatement, here from the kernels, which equal it bit for bit
usage: mesh_smooth_cost.py [OUT_STEM]      mesh_smooth_cost.py --md STEM   (the table of a run's .json written again)"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from levelsetfusion_python_amd import _lib, device_mesh_smooth as D  # noqa: E402
from levelsetfusion_python_amd.device_core import stream_ptr  # noqa: E402

VOXEL = 0.004
ITERATIONS = D.DEFAULT_ITERATIONS
PASSES = 2 * ITERATIONS


class Launches:
    """the three foreign calls of device_mesh_smooth.smooth on workspaces and outputs allocated once"""

    def __init__(self, v, f):
        self.c = D.prepare(v, f, ITERATIONS)
        self.out = D.run(self.c)
        self.sums = torch.empty((max(self.c.V, 1), 3), dtype=torch.int64, device=v.device)
        self.normals = torch.empty((self.c.V, 3), dtype=torch.float32, device=v.device)
        c = self.c
        self.workspace_bytes = sum(t.numel() * t.element_size() for t in (
            c.vertex_work, c.edge_keys, c.edge_counts, c.tile_offsets, c.neighbours, c.scratch, self.sums))

    @staticmethod
    def _ptrs(*ts):
        return [ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None for t in ts]

    def prepare(self):
        c = self.c
        _lib.check(_lib.lib.lsf_mesh_smooth_prepare(
            *self._ptrs(c.vertices, c.faces, c.vertex_work, c.edge_keys, c.edge_counts, c.tile_offsets, c.neighbours,
                        c.scalars, c.record), c.P, stream_ptr()), "lsf_mesh_smooth_prepare")

    def run(self):
        c = self.c
        _lib.check(_lib.lib.lsf_mesh_smooth_run(
            *self._ptrs(c.vertices, c.vertex_work, c.neighbours, self.out, c.scratch, c.scalars, c.record), c.P,
            stream_ptr()), "lsf_mesh_smooth_run")

    def vertex_normals(self):
        c = self.c
        _lib.check(_lib.lib.lsf_mesh_vertex_normals(
            *self._ptrs(self.out, c.faces, self.sums, self.normals, c.scalars, c.record), c.P, stream_ptr()),
            "lsf_mesh_vertex_normals")

    def pass_bytes(self):
        """bytes one pass reads and writes at least once, gathers counted by their words: per vertex its position read
        and written (24), its degree, pin and row offset (12); per neighbour-list entry the index (4) and the gathered
        position (12)"""
        return self.c.V * 36 + 2 * self.c.rec["edges"] * 16

    def torch_pair(self):
        """a lambda | mu pass pair with torch.index_add_ on the same edges, degrees and pins, in float32"""
        c = self.c
        keys = c.edge_keys[c.edge_keys >= 0]
        lo, hi = keys >> 32, keys & 0xffffffff
        degree, pinned = c.vertex_work[0, :c.V], c.vertex_work[1, :c.V]
        moves = ((pinned == 0) & (degree > 0))[:, None]
        inverse = (1.0 / degree.clamp(min=1).to(torch.float32))[:, None]

        def one(p, w):
            s = torch.zeros_like(p)
            s.index_add_(0, lo, p[hi])
            s.index_add_(0, hi, p[lo])
            return torch.where(moves, p + w * (s * inverse - p), p)

        return lambda: one(one(c.vertices, D.DEFAULT_LAM), D.DEFAULT_MU)


def rows():
    import mesh_cost
    import mesh_simplify_cost
    from levelsetfusion_python_amd import device_mesh_components, device_mesh_simplify
    out = []
    for name, (vol, off) in (("synthetic frame 256³", mesh_cost.model(256)),
                             ("padded noise 128³", mesh_simplify_cost.noise_model(128))):
        extract_ms = mesh_cost.best_wall_ms(lambda: vol.extract_mesh(off, VOXEL, normals=True, as_tensor=True))
        v, f, n = vol.extract_mesh(off, VOXEL, normals=True, as_tensor=True)
        weld_ms = mesh_cost.best_wall_ms(lambda: device_mesh_simplify.simplify(v, f, n, None, None))
        filter_ms = mesh_cost.best_wall_ms(lambda: device_mesh_components.filter(v, f, n, None, keep_largest=1))
        run = Launches(v, f)
        device = {step: mesh_cost.best_ms(getattr(run, step)) for step in ("prepare", "run", "vertex_normals")}
        torch_pair_ms = mesh_cost.best_ms(run.torch_pair())
        call_ms = mesh_cost.best_wall_ms(lambda: D.smooth(v, f, n, None))
        both_ms = mesh_cost.best_wall_ms(lambda: vol.extract_mesh(off, VOXEL, normals=True, as_tensor=True,
                                                                  smooth_iterations=ITERATIONS))
        rec = D.smooth(v, f, n, None, return_record=True)[4]
        pass_ms = device["run"] / PASSES
        total_ms = sum(device.values())
        row = dict(model=name, iterations=ITERATIONS, passes=PASSES, record=rec,
                   table_slots=run.c.p.table_slots, workspace_bytes=run.workspace_bytes,
                   prepare_us=device["prepare"] * 1e3, run_us=device["run"] * 1e3, pass_us=pass_ms * 1e3,
                   normals_us=device["vertex_normals"] * 1e3, smooth_call_wall_us=call_ms * 1e3,
                   smooth_host_us=(call_ms - total_ms) * 1e3, weld_call_wall_us=weld_ms * 1e3,
                   filter_call_wall_us=filter_ms * 1e3, extract_call_wall_us=extract_ms * 1e3,
                   extract_with_smooth_wall_us=both_ms * 1e3, pass_bytes=run.pass_bytes(),
                   pass_tb_s=run.pass_bytes() / (pass_ms * 1e-3) / 1e12, hip_pair_us=2 * pass_ms * 1e3,
                   torch_pair_us=torch_pair_ms * 1e3)
        out.append(row)
        print(json.dumps(row), flush=True)
        del run, vol, v, f, n
        torch.cuda.empty_cache()
    return out


def sphere_figures():
    """the figures of the 24^3 test sphere, from the kernels"""
    import mesh_smooth_scenes as T
    from levelsetfusion_python_amd import fusion
    v, f, n = T.sphere_mesh(True)
    out = dict(vertices=len(v), faces=len(f), input_radius_std=T.radius_std(v), runs=[])
    for label, iterations, mu in (("Taubin, 10 iterations", 10, D.DEFAULT_MU), ("Taubin, 30 iterations", 30, D.DEFAULT_MU),
                                  ("Laplacian, 10 iterations", 10, 0.0)):
        p = fusion.smooth_mesh((v, f), iterations, mu=mu)[0]
        out["runs"].append(dict(run=label, radius_std=T.radius_std(p), volume_ratio=T.volume(p, f) / T.volume(v, f)))
    cv, cf, cn = T.sphere_mesh(False)
    p, _, pn = fusion.smooth_mesh((cv, cf, cn), 10)
    out["clean_sphere"] = dict(vertices=len(cv), faces=len(cf), volume_ratio=T.volume(p, cf) / T.volume(cv, cf),
                               least_normal_dot=float((fusion.mesh_vertex_normals((cv, cf)).astype(np.float64)
                                                       * cn).sum(axis=1).min()),
                               least_normal_dot_smoothed=float((pn.astype(np.float64) * cn).sum(axis=1).min()))
    print(json.dumps(out), flush=True)
    return out


# what the committed run showed
NOTES = """## Reading

One run of the tool.  Nobody had measured any of this before; these are first figures, not a floor, and no kernel was
traced on its own, so what is said about single kernels below is supposition.

A pass on the large mesh (3.0 M vertices, 9.7 M edges) takes 0.235 ms and moves the bytes counted for it at 1.77 TB/s,
of the 6.3 TB/s a copy reaches.  It is bound by the gather: per neighbour a 4-byte index and a 12-byte position from
wherever that vertex lies, a fraction of every cache line it touches; the mesh is in voxel order, so most neighbours are
near in memory and hit in cache, which is why the counted rate is as high as it is.  How much of the time the float64 arithmetic takes (three
conversions and roundings per neighbour, three divisions per vertex) was not measured apart.  On the small mesh a pass
takes 13.8 µs for 6 MB, 0.45 TB/s: twenty dependent launches of 183 tiles each, bound by launch and latency, not by bytes.

`prepare` costs as much as 17 passes on the large mesh (4.0 ms) and 7.5 on the small one (0.10 ms).  Its table has
67 M slots of 12 bytes for 9.7 M edges -- the power of two above 2 · 3F, 14 % full -- and is filled once and walked twice
(the edge counts and pins, then the neighbour list): 2.4 GB of table traffic next to 19 M compare-and-swaps and 39 M
atomic adds.  A table sized from the edge count, or keys kept per face and sorted, would cut it; neither was tried.
The normals take 2.35 ms on the large mesh, ten passes' worth: nine 64-bit atomic adds per face, 58 M in all, on sums
that neighbours share.  A gather over the faces around a vertex would replace them by loads and needs a second
compressed-row list; not tried.

The whole call is 11.2 ms on the large mesh -- 3.1 times `filter_mesh_components` (3.7 ms), 7.9 times welding (1.4 ms)
and 36 times the extraction that made the mesh (0.31 ms) -- and 0.48 ms on the small one, next to 0.55 ms for the filter,
0.17 ms for welding and 0.41 ms for the extraction; `extract_mesh` with `smooth_iterations=10` takes 0.87 ms there.
`host` is a difference of best-of-10 figures taken in separate loops: 0.05 ms small, 0.16 ms large.

What the HIP path buys: a λ | μ pass pair written with `torch.index_add_` on the same edge list takes 3.13 ms on the
large mesh and 0.113 ms on the small one, against 0.47 ms and 0.028 ms for two passes here, 6.6 and 4.1 times as long,
and its float32 atomic sums are not the same bits from run to run, where the integer sums here are."""


def write_md(path, data, notes=None):
    notes = NOTES if notes is None else notes
    lines = ["# Cost of mesh smoothing (MI355X)", "",
             "`tools/mesh_smooth_cost.py` (raw numbers: `mesh_smooth_cost.json`).  The two meshes of",
             "`mesh_simplify_cost.md`, both with normals: the mesh of `tools/mesh_cost.py`'s 256³ model (one synthetic",
             "depth frame fused, an open sheet whose border is pinned) and the mesh of a padded-noise 128³ volume (4 mm",
             "voxels, closed), each smoothed by the default %d Taubin iterations, %d passes.  `prepare`, `run` and"
             % (ITERATIONS, PASSES),
             "`normals` are the launches of `lsf_mesh_smooth_prepare`, `_run` and `lsf_mesh_vertex_normals`, each call",
             "timed with events on workspaces allocated once, best of 10; `pass` is `run` by its passes.  `call` is",
             "`device_mesh_smooth.smooth` (all three, one host read) on device tensors between device synchronisations,",
             "best of 10; `host` = call - the three device parts is the read of the record, the allocations and Python.",
             "`weld` is `device_mesh_simplify.simplify` welding the same mesh, `filter` is",
             "`device_mesh_components.filter(keep_largest=1)` and `extract` is `extract_mesh(normals=True,",
             "as_tensor=True)` on the same model, all in the same run; `both` is `extract_mesh` with",
             "`smooth_iterations=%d`.  Pass bytes: what one pass reads and writes at least once (the tool's" % ITERATIONS,
             "`pass_bytes`), gathers counted by their words, not their cache lines.  `torch pair` is a λ | μ pass pair",
             "written with `torch.index_add_` on the same edge list in float32, next to two passes of the HIP path.", "",
             "| mesh | V | F | E | border edges | pinned | max degree | prepare | run | pass | normals | call | host "
             "| weld | filter | extract | both | workspaces | pass bytes | pass TB/s | HIP pair | torch pair |",
             "|" + "---|" * 22]
    for r in data["mesh_smooth"]:
        rec = r["record"]
        lines.append("| %s | %d | %d | %d | %d | %d | %d | %.1f µs | %.1f µs | %.2f µs | %.1f µs | %.1f µs | %.1f µs "
                     "| %.1f µs | %.1f µs | %.1f µs | %.1f µs | %.1f MB | %.2f MB | %.3f | %.1f µs | %.1f µs |"
                     % (r["model"], rec["vertices_in"], rec["faces_in"], rec["edges"], rec["boundary_edges"],
                        rec["pinned_vertices"], rec["max_degree"], r["prepare_us"], r["run_us"], r["pass_us"],
                        r["normals_us"], r["smooth_call_wall_us"], r["smooth_host_us"], r["weld_call_wall_us"],
                        r["filter_call_wall_us"], r["extract_call_wall_us"], r["extract_with_smooth_wall_us"],
                        r["workspace_bytes"] / 1e6, r["pass_bytes"] / 1e6, r["pass_tb_s"], r["hip_pair_us"],
                        r["torch_pair_us"]))
    s = data["test_sphere"]
    lines += ["", "## The test sphere", "",
              "The 24³ test sphere of `tests/mesh_smooth_scenes.py` (radius 6.3, band 3, noise 0.35 · standard normal on",
              "the distance; %d vertices, %d faces, closed), smoothed by `fusion.smooth_mesh`: the kernels' float32"
              % (s["vertices"], s["faces"]),
              "figures, which `tests/test_mesh_smooth_host.py` asserts on the restatement.", "",
              "| run | std of vertex radius | volume ratio |", "|---|---|---|",
              "| input | %.5f | — |" % s["input_radius_std"]]
    lines += ["| %s | %.5f | %.5f |" % (r["run"], r["radius_std"], r["volume_ratio"]) for r in s["runs"]]
    c = s["clean_sphere"]
    lines += ["", "On the clean sphere (%d vertices, %d faces) ten Taubin iterations give a volume ratio of %.5f; the least"
              % (c["vertices"], c["faces"], c["volume_ratio"]),
              "dot product of a normal rebuilt from the faces with the extraction's gradient normal is %.5f before and"
              % c["least_normal_dot"], "%.5f after them." % c["least_normal_dot_smoothed"], ""]
    if notes:
        lines += [notes, ""]
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--md":  # the table of a run's .json written again, after NOTES changed
        with open(sys.argv[2] + ".json") as f:
            write_md(sys.argv[2] + ".md", json.load(f))
        return
    data = dict(mesh_smooth=rows(), test_sphere=sphere_figures())
    stem = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mesh_smooth_cost")
    with open(stem + ".json", "w") as f:
        json.dump(data, f, indent=1)
    write_md(stem + ".md", data)


if __name__ == "__main__":
    main()
