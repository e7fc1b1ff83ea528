"""Cost of mesh extraction (profiles/mesh_cost.md, .json) on the synthetic depth frame fused into the model
(synthetic.depth_image, K = [[700, 0, 320], [0, 700, 240], [0, 0, 1]], 4 mm voxels, the surface at 1 m in the middle of
the volume, 20-voxel band), at 128^3, 256^3 and 512^3, without and with normals:
  * the counting launches (lsf_mesh_count) and the emitting launches (lsf_mesh_emit), each timed with events on
    workspaces allocated once, best of 10 after a warm-up
  * the whole public call (CanonicalVolume.extract_mesh with as_tensor=True) between device synchronisations, best of
    10: what is left after the two device parts is the host read of the totals, the output allocation and Python
  * V and F, and the bytes the launches move against the floor of reading tsdf and weight once (8 B/voxel)
usage: mesh_cost.py [OUT_STEM]        mesh_cost.py --trace N    (one call of each kind, for rocprofv3)"""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import levelsetfusion_python_amd as lsf  # noqa: E402
from levelsetfusion_python_amd import _lib, device_mesh, synthetic  # noqa: E402
from levelsetfusion_python_amd.device_core import stream_ptr  # noqa: E402
from levelsetfusion_python_amd.tsdf import generation as gen  # noqa: E402

K = np.array([[700.0, 0, 320], [0, 700.0, 240], [0, 0, 1]], dtype=np.float32)
CAM = gen.DepthCamera(intrinsics=gen.DepthCamera.Intrinsics(intrinsic_matrix=K))
HBM_TB_S = 6.3  # the achievable HBM bandwidth of an MI355X (float4 copy)


def model(n):
    off = np.array([-n // 2, -n // 2, 250 - n // 2])
    vol = lsf.fusion.CanonicalVolume(n)
    vol.integrate_depth(synthetic.depth_image(), CAM, np.zeros(6), off)
    torch.cuda.synchronize()
    return vol, off


def best_ms(fn, reps=10):
    fn()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def best_wall_ms(fn, reps=10):
    fn()
    best = float("inf")
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t) * 1e3)
    return best


class Launches:
    """the two halves of device_mesh.extract_mesh on workspaces and outputs allocated once"""

    def __init__(self, vol, off, normals):
        self.p = device_mesh.params(tuple(vol.tsdf.shape), off)
        n = vol.tsdf.numel()
        blocks = (n + _lib.MESH_TILE - 1) // _lib.MESH_TILE
        d = vol.tsdf.device
        self.vol = vol
        self.code = torch.empty(n, dtype=torch.uint8, device=d)
        self.mask = torch.empty(n, dtype=torch.uint8, device=d)
        self.offsets = torch.empty(2 * blocks, dtype=torch.int32, device=d)
        self.totals = torch.empty(2, dtype=torch.int64, device=d)
        self.base = torch.empty(n, dtype=torch.int32, device=d)
        self.count()
        self.v, self.f = (int(x) for x in self.totals.tolist())
        self.verts = torch.empty((self.v, 3), dtype=torch.float32, device=d)
        self.faces = torch.empty((self.f, 3), dtype=torch.int32, device=d)
        self.normals = torch.empty((self.v, 3), dtype=torch.float32, device=d) if normals else None

    def _ptrs(self, *ts):
        return [ctypes.c_void_p(t.data_ptr()) if t is not None else None for t in ts]

    def count(self):
        _lib.check(_lib.lib.lsf_mesh_count(*self._ptrs(self.vol.tsdf, self.vol.weight, self.code, self.mask,
                                                       self.offsets, self.totals), ctypes.byref(self.p),
                                           stream_ptr()), "lsf_mesh_count")

    def emit(self):
        _lib.check(_lib.lib.lsf_mesh_emit(*self._ptrs(self.vol.tsdf, self.vol.weight, self.code, self.mask,
                                                      self.offsets, self.base, self.verts, self.normals, self.faces),
                                          self.v, self.f, ctypes.byref(self.p), stream_ptr()), "lsf_mesh_emit")


def moved_bytes(n, v, f, normals):
    """bytes the five launches read and write at least once: counting 8 (tsdf, weight) + 1 (code) + 1 (code) + 1 (mask)
    per voxel; emitting 1 (mask) + 1 (code) per voxel, per vertex its base, position, two end values (and with normals
    12 more bytes and the neighbours, not counted), per face 12 bytes"""
    voxels = n ** 3
    return voxels * 13 + v * (4 + 12 + 8 + (12 if normals else 0)) + f * 12


def rows():
    out = []
    for n in (128, 256, 512):
        vol, off = model(n)
        for normals in (False, True):
            run = Launches(vol, off, normals)
            count_ms = best_ms(run.count)
            emit_ms = best_ms(run.emit)
            call_ms = best_wall_ms(lambda: vol.extract_mesh(off, normals=normals, as_tensor=True))
            moved = moved_bytes(n, run.v, run.f, normals)
            floor_us = 8 * n ** 3 / (HBM_TB_S * 1e12) * 1e6
            row = dict(n=n, normals=normals, vertices=run.v, faces=run.f, count_us=count_ms * 1e3,
                       emit_us=emit_ms * 1e3, call_wall_us=call_ms * 1e3,
                       host_us=(call_ms - count_ms - emit_ms) * 1e3, bytes_moved=moved,
                       floor_bytes=8 * n ** 3, floor_us=floor_us,
                       device_tb_s=moved / ((count_ms + emit_ms) * 1e-3) / 1e12)
            out.append(row)
            print(json.dumps(row), flush=True)
            del run
        del vol
        torch.cuda.empty_cache()
    return out


def write_md(path, table):
    lines = ["# Cost of mesh extraction (MI355X)", "",
             "`tools/mesh_cost.py` (raw numbers: `mesh_cost.json`; one call without and one with normals at 256³ "
             "under",
             "`rocprofv3 --kernel-trace --stats`: `mesh_kernel_stats.csv`).  The model holds the fused frame",
             "`synthetic.depth_image()` (4 mm voxels, the surface at 1 m in the middle of the volume, 20-voxel band).",
             "`count` is the three counting launches and `emit` the two emitting launches, each timed with events on",
             "workspaces allocated once, best of 10.  `call` is `extract_mesh(..., as_tensor=True)` between device",
             "synchronisations, best of 10; `host` = call - count - emit is the read of the two totals, the output",
             "allocation and Python.  Bytes moved: 13 B per voxel (tsdf and weight read, the cell codes written and",
             "read twice, the edge masks written and read) plus the vertices' and faces' own bytes.  Floor: tsdf and",
             "weight read once, 8 B/voxel at %.1f TB/s." % HBM_TB_S, "",
             "| volume | normals | V | F | count | emit | call | host | bytes moved | floor (8 B/voxel) "
             "| device TB/s |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in table:
        row = "| %d³ | %s | %d | %d | %.1f µs | %.1f µs | %.1f µs | %.1f µs | %.1f MB | %.1f µs | %.2f |"
        lines.append(row % (r["n"], "yes" if r["normals"] else "no", r["vertices"], r["faces"], r["count_us"],
                            r["emit_us"], r["call_wall_us"], r["host_us"], r["bytes_moved"] / 1e6, r["floor_us"],
                            r["device_tb_s"]))
    lines.append("")
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--trace":
        n = int(sys.argv[2])
        vol, off = model(n)
        sizes = [[len(a) for a in vol.extract_mesh(off, normals=normals, as_tensor=True)] for normals in (False, True)]
        torch.cuda.synchronize()
        print(json.dumps(dict(n=n, sizes=sizes)))
        return
    table = rows()
    stem = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mesh_cost")
    with open(stem + ".json", "w") as f:
        json.dump(dict(mesh=table), f, indent=1)
    write_md(stem + ".md", table)


if __name__ == "__main__":
    main()
