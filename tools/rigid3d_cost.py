"""Cost of the 6-DoF SDF-2-SDF rigid 3-D tracker (profiles/rigid3d_cost.md) at 64^3, 128^3 and 256^3 on the synthetic
depth frames (synthetic.depth_image, 4 mm voxels, surface at 1 m):
  * device time per iteration: the slope between enqueued runs of 10 and 60 iterations (events around
    device_rigid.rigid_run_3d, best of 5), so the finishing launch and the copy back drop out; voxels/s from it
  * wall time of one Sdf2SdfOptimizer3d.optimize(iteration=60): canonical volume, depth upload, 61 launches, copy back
  * the composed path per iteration: the typed generator (live volume), calculate_gradient_wrt_twist_3d, torch sums of
    A, b and the energy, a copy to the host and a numpy solve -- and its ratio to the fused path
usage: rigid3d_cost.py [OUT_JSON]       rigid3d_cost.py --trace N ITERATIONS   (one call, for rocprofv3)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import levelsetfusion_python_amd as lsf  # noqa: E402
from levelsetfusion_python_amd import device_rigid, synthetic  # noqa: E402
from levelsetfusion_python_amd.rigid_opt.sdf_generation import ArrayBasedSingleFrameDataset  # noqa: E402
from levelsetfusion_python_amd.rigid_opt.sdf_gradient_field import calculate_gradient_wrt_twist_3d  # noqa: E402
from levelsetfusion_python_amd.tsdf import generation as gen  # noqa: E402

K = np.array([[700.0, 0, 320], [0, 700.0, 240], [0, 0, 1]], dtype=np.float32)
CAM = gen.DepthCamera(intrinsics=gen.DepthCamera.Intrinsics(intrinsic_matrix=K))


def case(n):
    d0, d1 = synthetic.depth_image(), synthetic.depth_image(shift_px=2.0, nearer_m=0.008)
    off = np.array([-n // 2, -n // 2, 250 - n // 2])
    data = ArrayBasedSingleFrameDataset(d0, d1, 240, n, off, CAM)
    canonical = data.generate_3d_canonical_field(as_tensor=True)
    depth, code = gen.device_depth(d1)
    return data, canonical, depth, code, d1, off


def run_ms(canonical, depth, code, off, iterations, reps=5):
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        device_rigid.rigid_run_3d(canonical, depth, code, CAM, off, iterations, 0.5, 0.01, 0.004, 0.004, 20.)
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def composed_iteration(canonical, d1, off, twist, n, eta=0.01):
    """one iteration without the fused kernel: generator, gradient kernel, torch sums, host solve"""
    live = gen.generate_tsdf_field_from_depth_image_typed(
        d1, CAM, None, lsf.transformation.twist_vector_to_matrix3d(twist.astype(np.float32)), field_size=n,
        array_offset=off, dims=3, as_tensor=True)
    g = calculate_gradient_wrt_twist_3d(live, twist, off, 0.004, as_tensor=True).reshape(-1, 6)
    c, l = canonical.reshape(-1), live.reshape(-1)
    a = torch.empty((6, 6), dtype=torch.float64, device="cuda")
    for i in range(6):
        for j in range(i, 6):
            a[i, j] = a[j, i] = (g[:, i] * g[:, j]).double().sum()
    gd = g.double()
    dot = gd[:, 0] * float(twist[0])
    for i in range(1, 6):
        dot = dot + gd[:, i] * float(twist[i])
    r = (c - l).double() + dot
    b = (r[:, None] * gd).sum(0)
    d = c.double() * (c > -eta) - l.double() * (l > -eta)
    energy = 0.5 * (d * d).sum()
    a, b, energy = a.cpu().numpy(), b.cpu().numpy(), float(energy)
    return twist + 0.5 * (np.linalg.inv(a).dot(b) - twist)


def composed_ms(canonical, d1, off, n, iterations=5):
    twist = np.zeros(6)
    composed_iteration(canonical, d1, off, twist, n)  # warm-up
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iterations):
        twist = composed_iteration(canonical, d1, off, twist, n)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / iterations


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--trace":
        n, iterations = int(sys.argv[2]), int(sys.argv[3])
        data, canonical, depth, code, _, off = case(n)
        opt = lsf.Sdf2SdfOptimizer3d()
        opt.optimize(data, iteration=iterations)
        torch.cuda.synchronize()
        twist = opt.optimize(data, iteration=iterations)
        print(json.dumps(dict(n=n, iterations=iterations, twist=twist.ravel().tolist())))
        return
    rows = []
    for n in (64, 128, 256):
        data, canonical, depth, code, d1, off = case(n)
        run_ms(canonical, depth, code, off, 10, 2)  # warm-up
        t10, t60 = run_ms(canonical, depth, code, off, 10), run_ms(canonical, depth, code, off, 60)
        per_it = (t60 - t10) / 50
        opt = lsf.Sdf2SdfOptimizer3d()
        opt.optimize(data, iteration=60)
        walls = []
        for _ in range(3):
            torch.cuda.synchronize()
            t = time.perf_counter()
            twist = opt.optimize(data, iteration=60)
            walls.append((time.perf_counter() - t) * 1e3)
        comp = composed_ms(canonical, d1, off, n)
        tiles = ((n + 15) // 16) ** 2
        zc = min(n, max(4, -(-n * tiles // 256)))
        items = tiles * -(-n // zc)
        rows.append(dict(n=n, workgroups=min(items, 256), z_chunk=zc, device_ms_per_iteration=per_it, run_ms_10=t10,
                         run_ms_60=t60, voxels_per_s=n ** 3 / (per_it * 1e-3), optimize_wall_ms_60=min(walls),
                         composed_ms_per_iteration=comp, composed_over_fused=comp / per_it,
                         final_twist=twist.ravel().tolist(), last_energy=opt.last_records[-1]["energy"],
                         first_energy=opt.last_records[0]["energy"]))
        print(json.dumps(rows[-1]), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
