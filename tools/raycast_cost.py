"""Cost of ray-casting the canonical TSDF (profiles/raycast_cost.md, .json) on the synthetic depth frame
(synthetic.depth_image, K = [[700, 0, 320], [0, 700, 240], [0, 0, 1]], 4 mm voxels, the surface at 1 m in the middle of
the volume, 20-voxel band):
  * device time of one 640 x 480 ray-cast, without and with normals, at 128^3, 256^3 and 512^3 models that hold one
    fused frame: events around device_raycast.raycast, best of 10 after a warm-up; the hit count; a bytes-touched
    estimate (the tsdf and weight of every voxel, read once, plus the images written)
  * the per-frame split of SequenceFusion3d.integrate in both tracking modes at 128^3 and 256^3 (the second frame:
    the ray-cast, the prediction's live volume, the rigid run with its copy back, the fusion with its record read), each
    step timed between device synchronisations, best of 3 by whole-frame wall time
usage: raycast_cost.py [OUT_STEM]        raycast_cost.py --trace N    (one ray-cast of each kind, for rocprofv3)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import levelsetfusion_python_amd as lsf  # noqa: E402
from levelsetfusion_python_amd import _lib, device_fusion, device_raycast, device_rigid, synthetic  # noqa: E402
from levelsetfusion_python_amd.tsdf import generation as gen  # noqa: E402

K = np.array([[700.0, 0, 320], [0, 700.0, 240], [0, 0, 1]], dtype=np.float32)
CAM = gen.DepthCamera(intrinsics=gen.DepthCamera.Intrinsics(intrinsic_matrix=K))
METRIC = gen.DepthCamera(intrinsics=gen.DepthCamera.Intrinsics(intrinsic_matrix=K), depth_unit_ratio=1.0)
TWIST = np.array([0.001, -0.001, 0.002, 0.002, -0.003, 0.001])


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


def cast(vol, off, normals):
    return device_raycast.raycast(vol.tsdf, vol.weight, CAM, TWIST, off, normals=normals)


def raycast_rows():
    rows = []
    for n in (128, 256, 512):
        vol, off = model(n)
        hits = int(cast(vol, off, False)[2].item())
        for normals in (False, True):
            ms = best_ms(lambda: cast(vol, off, normals))
            moved = 8 * n ** 3 + 640 * 480 * (16 if normals else 4)
            rows.append(dict(n=n, normals=normals, device_us=ms * 1e3, hits=hits, volume_bytes=8 * n ** 3,
                             bytes_touched=moved, effective_tb_s=moved / (ms * 1e-3) / 1e12))
            print(json.dumps(rows[-1]), flush=True)
        del vol
        torch.cuda.empty_cache()
    return rows


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e3


def split_rows(rigid_iterations=60):
    rows = []
    d0, d1 = synthetic.depth_image(), synthetic.depth_image(shift_px=2.0, nearer_m=0.008)
    for n in (128, 256):
        off = np.array([-n // 2, -n // 2, 250 - n // 2])
        for mode in ("model", "raycast"):
            best = None
            for _ in range(3):
                seq = lsf.SequenceFusion3d(CAM, n, off, rigid_iterations=rigid_iterations, tracking_reference=mode)
                seq.integrate(d0)
                m = seq.canonical
                prev, prev_code = gen.device_depth(d0)
                depth, code = gen.device_depth(d1)
                cast_ms = live_ms = 0.0
                reference = m.tsdf
                if mode == "raycast":
                    (pred, _, _), cast_ms = timed(lambda: device_raycast.raycast(
                        m.tsdf, m.weight, CAM, np.zeros(6), off, image_shape=tuple(prev.shape), fallback_depth=prev,
                        fallback_code=prev_code))
                    reference, live_ms = timed(lambda: device_rigid.live_volume_3d(
                        pred, _lib.DEPTH_F32, METRIC, (n,) * 3, off, np.zeros(6)))
                (twist, _), rigid = timed(lambda: device_rigid.rigid_run_3d(
                    reference, depth, code, CAM, off, rigid_iterations, 0.5, 0.01, 0.004, 0.004, 20,
                    twist=np.zeros(6)))
                t_, w_ = m.tsdf.clone(), m.weight.clone()
                _, fuse = timed(lambda: device_fusion.integrate_depth(t_, w_, depth, code, CAM, off, twist).cpu())
                _, whole = timed(lambda: seq.integrate(d1))
                row = dict(n=n, tracking_reference=mode, raycast_ms=cast_ms, prediction_volume_ms=live_ms,
                           rigid_ms=rigid, fuse_ms=fuse, integrate_wall_ms=whole, rigid_iterations=rigid_iterations,
                           prediction_hits=seq.frame_records[-1]["prediction_hits"])
                if best is None or row["integrate_wall_ms"] < best["integrate_wall_ms"]:
                    best = row
            rows.append(best)
            print(json.dumps(best), flush=True)
    return rows


def write_md(path, cast_rows, split):
    lines = ["# Cost of ray-casting the canonical TSDF (MI355X)", "",
             "`tools/raycast_cost.py` (raw numbers: `raycast_cost.json`; one ray-cast without and one with normals at "
             "256³", "under `rocprofv3 --kernel-trace --stats`: `raycast_kernel_stats.csv`).  The model holds the "
             "fused frame", "`synthetic.depth_image()` (4 mm voxels, the surface at 1 m in the middle of the volume, "
             "20-voxel band); the", "camera is 640 x 480 at a small twist.  Device time is one launch, events around "
             "it, best of 10.  Bytes touched:", "the tsdf and weight of every voxel read once (8 B/voxel) plus the "
             "images written, an upper bound on the", "unique bytes, since rays only visit voxels in the view and "
             "stop at the surface; the march re-reads cached", "lines many times over (8 weights, and 8 tsdf values "
             "where all weights are > 0, per half-voxel step).", "",
             "| volume | normals | device / call | hits | bytes touched | effective TB/s |", "|---|---|---|---|---|---|"]
    for r in cast_rows:
        lines.append("| %d³ | %s | %.1f µs | %d | %.1f MB | %.2f |" % (
            r["n"], "yes" if r["normals"] else "no", r["device_us"], r["hits"], r["bytes_touched"] / 1e6,
            r["effective_tb_s"]))
    lines += ["", "**Per-frame split** of `SequenceFusion3d.integrate` (the second frame; each step timed between "
              "device", "synchronisations, so host work is included; best of 3 by whole-frame wall time; %d rigid "
              "iterations, no" % split[0]["rigid_iterations"], "non-rigid step):", "",
              "| volume | tracking_reference | ray-cast | prediction's live volume | rigid run | fuse + record read "
              "| `integrate()` wall |", "|---|---|---|---|---|---|---|"]
    for r in split:
        lines.append("| %d³ | %s | %.3f ms | %.3f ms | %.2f ms | %.3f ms | %.2f ms |" % (
            r["n"], r["tracking_reference"], r["raycast_ms"], r["prediction_volume_ms"], r["rigid_ms"], r["fuse_ms"],
            r["integrate_wall_ms"]))
    lines.append("")
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--trace":
        n = int(sys.argv[2])
        vol, off = model(n)
        hits = [int(cast(vol, off, normals)[2].item()) for normals in (False, True)]
        print(json.dumps(dict(n=n, hits=hits)))
        return
    cast_rows = raycast_rows()
    split = split_rows()
    stem = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "raycast_cost")
    with open(stem + ".json", "w") as f:
        json.dump(dict(raycast=cast_rows, frame_split=split), f, indent=1)
    write_md(stem + ".md", cast_rows, split)


if __name__ == "__main__":
    main()
