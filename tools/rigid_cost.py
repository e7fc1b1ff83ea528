"""Cost of the SDF-2-SDF rigid tracker (profiles/rigid_cost.md): device time per iteration and wall time per
Sdf2SdfOptimizer2d.optimize() at 32^2 ... 1024^2 on the reference's two EXR frames, against the numpy restatement's CPU
time for the same call (tests/rigid_restatement.py -- a vectorised restatement, not the reference's per-voxel loop).
Device time per iteration is the slope between two iteration counts of one enqueued run (events around
device_rigid.rigid_run), so the fixed cost of the finishing launch and the copy back drops out.
usage: rigid_cost.py [OUT_JSON]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import levelsetfusion_python_amd as lsf  # noqa: E402
from levelsetfusion_python_amd import device_rigid, image_io  # noqa: E402
from levelsetfusion_python_amd.rigid_opt.sdf_generation import ArrayBasedSingleFrameDataset  # noqa: E402
from levelsetfusion_python_amd.tsdf.generation import DepthCamera, FilteringMethod, device_depth  # noqa: E402
import rigid_restatement as R  # noqa: E402

K = np.array([[570.3999633789062, 0, 320], [0, 570.3999633789062, 240], [0, 0, 1]], dtype=np.float32)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def run_ms(data, canonical, depth, code, iterations, reps=5):
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        device_rigid.rigid_run(canonical, depth, code, data.depth_camera, 240, data.offset, iterations, 0.5, 0.01,
                               0.004, 0.004, 20.)
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def main():
    d0 = image_io.read_depth_image(os.path.join(GOLDEN, "depth_000000.exr"))
    d1 = image_io.read_depth_image(os.path.join(GOLDEN, "depth_000003.exr"))
    cam = DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=K))
    rows = []
    for n in (32, 128, 512, 1024):
        off = np.array([-n / 2, -n / 2, 112.0 - n / 2 * (128 / n if n > 128 else 1)])
        data = ArrayBasedSingleFrameDataset(d0, d1, 240, n, off, cam)
        canonical = data.generate_2d_canonical_field(method=FilteringMethod.NONE, as_tensor=True)
        depth, code = device_depth(d1)
        run_ms(data, canonical, depth, code, 10, 2)  # warm-up
        t10, t60 = run_ms(data, canonical, depth, code, 10), run_ms(data, canonical, depth, code, 60)
        per_it = (t60 - t10) / 50
        opt = lsf.Sdf2SdfOptimizer2d()
        opt.optimize(data, iteration=60)
        walls = []
        for _ in range(3):
            torch.cuda.synchronize()
            t = time.perf_counter()
            opt.optimize(data, iteration=60)
            walls.append((time.perf_counter() - t) * 1e3)
        c_host = R.tsdf_nearest(d0, K, 0.001, (n, n), off, None, 20., 0.004, 240)
        t = time.perf_counter()
        R.optimize(c_host, d1, K, 0.001, 240, off, 60 if n <= 512 else 10, 20.)
        cpu = (time.perf_counter() - t) * 1e3 * (1 if n <= 512 else 6)
        tiles = ((n + 15) // 16) ** 2
        rows.append(dict(n=n, workgroups=min(tiles, 256), device_ms_per_iteration=per_it, run_ms_10=t10, run_ms_60=t60,
                         optimize_wall_ms_60=min(walls), restatement_cpu_ms_60=cpu))
        print(json.dumps(rows[-1]), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
