"""Cost of the Euclidean distance field (profiles/esdf_cost.md, .json) on tools/mesh_cost.py's model (one synthetic
depth frame fused) at 128^3 and 256^3, with max_distance_voxels R = 8, 32 and 64:
  * each pass of lsf_esdf_compute alone (the params' `passes`: x, y, z) and the three together, timed with events on
    scratch and outputs allocated once, over the scratch a whole call left, best of 10 after a warm-up
  * the whole public call (CanonicalVolume.esdf with as_tensor=True) between device synchronisations, best of 10: what
    is left after the launches is the host read of the record, the output allocation and Python
  * CanonicalVolume.extract_mesh and CanonicalVolume.raycast (480 x 640) on the same model in the same run, for scale
  * the bytes per voxel the passes move at least once, and the time that takes at the 8 TB/s of the HBM roofline
usage: esdf_cost.py [OUT_STEM]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mesh_cost  # noqa: E402
from levelsetfusion_python_amd import _lib, device_esdf as D  # noqa: E402

VOXEL = 0.004
SIZES = (128, 256)
RADII = (8, 32, 64)
HBM_TB_S = 8.0  # the roofline figure of README.md
# per voxel, each buffer counted once per pass: x reads tsdf and weight and writes the row offsets (its second sweep
# reads its own stores back through the caches); y reads the row offsets and writes the plane pairs; z reads the pairs,
# tsdf and weight and writes distance2, nearest and esdf
PASS_BYTES = {"x": 8 + 4, "y": 4 + 4, "z": 4 + 8 + 12}
PASSES = (("x", _lib.ESDF_PASS_X), ("y", _lib.ESDF_PASS_Y), ("z", _lib.ESDF_PASS_Z), ("all", _lib.ESDF_PASSES_ALL))


def rows():
    out = []
    for n in SIZES:
        vol, off = mesh_cost.model(n)
        extract_ms = mesh_cost.best_wall_ms(lambda: vol.extract_mesh(off, VOXEL, as_tensor=True))
        raycast_ms = mesh_cost.best_wall_ms(lambda: vol.raycast(mesh_cost.CAM, np.zeros(6), off, VOXEL, as_tensor=True))
        voxels = n ** 3
        for radius in RADII:
            worker = D.Esdf()
            _, distance2, nearest, record = worker.compute(vol.tsdf, vol.weight, VOXEL, radius)  # fills the scratch
            outputs = (distance2, nearest, torch.empty_like(vol.tsdf))
            times = {}
            for name, bits in PASSES:
                p = D.params((n, n, n), VOXEL, radius, passes=bits)
                times[name] = mesh_cost.best_ms(lambda: worker.enqueue(vol.tsdf, vol.weight, p, outputs)) * 1e3
            call_ms = mesh_cost.best_wall_ms(lambda: vol.esdf(VOXEL, radius, as_tensor=True))
            total_bytes = sum(PASS_BYTES.values()) * voxels
            far = voxels - record["finite"]
            row = dict(n=n, max_distance_voxels=radius, sites=record["sites"], finite=record["finite"], far=far,
                       max_distance2=record["max_distance2"], x_us=times["x"], y_us=times["y"], z_us=times["z"],
                       all_us=times["all"], call_wall_us=call_ms * 1e3, host_us=call_ms * 1e3 - times["all"],
                       extract_mesh_wall_us=extract_ms * 1e3, raycast_wall_us=raycast_ms * 1e3,
                       bytes_per_voxel=sum(PASS_BYTES.values()), floor_us=total_bytes / (HBM_TB_S * 1e12) * 1e6,
                       device_tb_s=total_bytes / (times["all"] * 1e-6) / 1e12,
                       pass_tb_s={k: PASS_BYTES[k] * voxels / (times[k] * 1e-6) / 1e12 for k in PASS_BYTES},
                       voxels_per_us=voxels / times["all"])
            out.append(row)
            print(json.dumps(row), flush=True)
            del worker, outputs, distance2, nearest
        del vol
        torch.cuda.empty_cache()
    return out


# what the committed table showed when it was measured
NOTES = """## Reading

The x pass does not depend on R: 115 µs at 256³, 12 B per voxel at 1.75 TB/s, a fifth of the roofline; it reads tsdf and
weight of seven voxels per voxel through the caches and reads its own forward sweep back.  At 128³ it takes 50 µs for an
eighth of the bytes: 16384 rows of two chunks each do not keep the card busy for long enough to stream.

The y and z passes are bound by the window length, not by bandwidth.  A voxel with a site nearby ends its walk after a
few steps; a voxel beyond the cap (`far`) walks all 2R + 1 rows or planes of its window and finds nothing.  The model
here is one fused frame, so most of the volume was never observed and lies far from the one surface: at 256³ 16.0 of
16.8 million voxels are beyond R = 8, and 8.4 million still beyond R = 64.  The y pass grows from 216 µs to 671 µs to
1310 µs for R = 8, 32, 64 and the z pass from 300 µs to 704 µs to 1168 µs: close to linear in R.  At R = 64 the y pass
spends 78 ps per voxel, 0.6 ps per voxel and window step, on reads that the vector L1 and the L2 serve (a step reads a
row that the lanes' neighbours in y read one step earlier or later); against the 8 B per voxel it has to move it runs
at 0.10 TB/s.  Each step is two loads and a few integer instructions, and the loop ends on a comparison with the
best distance so far, so as the code stands a lane has one step's loads in flight at a time.  A lower-envelope scan
(Meijster, Felzenszwalb) would make both passes independent of R; by the rule it must give the same bits.

The whole call at 256³ takes 0.63 ms at R = 8, 1.49 ms at R = 32 and 2.61 ms at R = 64, of which 31 to 39 µs are the host
(the record's read, three output allocations, Python).  That is 2.0, 4.7 and 8.3 times `extract_mesh` (0.31 ms) and
1.6, 3.8 and 6.7 times `raycast` (0.39 ms) on the same model, and 6.5, 16 and 28 times the 92 µs that 44 B per voxel
take at 8 TB/s.  These whole-call figures are what an incremental update after a fusion or a shift -- one that revisits
only the voxels within R of the sites that changed -- has to beat."""


def write_md(path, table, notes=NOTES):
    lines = ["# Cost of the Euclidean distance field (MI355X)", "",
             "`tools/esdf_cost.py` (raw numbers: `esdf_cost.json`).  The model holds the fused frame",
             "`synthetic.depth_image()` of `tools/mesh_cost.py` (4 mm voxels, the surface at 1 m in the middle of the",
             "volume, 20-voxel band).  `x`, `y`, `z` are the launches of `lsf_esdf_compute` one at a time (the params'",
             "`passes`), `all` the fill and the three launches of a whole call, each timed with events on scratch and",
             "outputs allocated once, best of 10 after a warm-up.  `call` is `CanonicalVolume.esdf(as_tensor=True)`",
             "between device synchronisations, best of 10; `host` = call - all is the read of the record, the output",
             "allocation and Python.  `extract_mesh` and `raycast` (480 x 640) are the public calls on the same model in",
             "the same run.  Bytes: %d B per voxel, every buffer counted once per pass (x %d, y %d, z %d); floor: that at"
             % (sum(PASS_BYTES.values()), PASS_BYTES["x"], PASS_BYTES["y"], PASS_BYTES["z"]),
             "%.0f TB/s.  `far` counts the voxels beyond the cap, which walk their whole window in the y and z passes." %
             HBM_TB_S, "",
             "| volume | R | sites | finite | far | x | y | z | all | call | host | floor | TB/s (all) | voxels/µs "
             "| extract_mesh | raycast |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in table:
        lines.append("| %d³ | %d | %d | %d | %d | %.1f µs | %.1f µs | %.1f µs | %.1f µs | %.1f µs | %.1f µs | %.1f µs "
                     "| %.2f | %.0f | %.1f µs | %.1f µs |"
                     % (r["n"], r["max_distance_voxels"], r["sites"], r["finite"], r["far"], r["x_us"], r["y_us"],
                        r["z_us"], r["all_us"], r["call_wall_us"], r["host_us"], r["floor_us"], r["device_tb_s"],
                        r["voxels_per_us"], r["extract_mesh_wall_us"], r["raycast_wall_us"]))
    lines.append("")
    if notes:
        lines += [notes, ""]
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    table = rows()
    stem = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "esdf_cost")
    with open(stem + ".json", "w") as f:
        json.dump(dict(esdf=table), f, indent=1)
    write_md(stem + ".md", table)


if __name__ == "__main__":
    main()
