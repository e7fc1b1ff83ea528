"""Cost of fusion into a canonical TSDF volume (profiles/fusion_cost.md, .json) on the synthetic depth frame
(synthetic.depth_image, K = [[700, 0, 320], [0, 700, 240], [0, 0, 1]], 4 mm voxels, the surface at 1 m in the middle of
the volume, 20-voxel band):
  * device time of one fuse call (both launches), volume mode and depth mode, at 128^3, 256^3 and 512^3: events around
    device_fusion.integrate_*, best of 10 after a warm-up, on a model that already holds one frame; bytes per voxel of
    the byte model and the fraction of 8 TB/s they imply
  * the per-frame split of SequenceFusion3d.integrate at 128^3 and 256^3 (the second frame: rigid run with its copy
    back, live volume, non-rigid optimize, fuse with its record read), each step timed between device synchronisations
usage: fusion_cost.py [OUT_STEM]        fusion_cost.py --trace N    (one call of each mode, for rocprofv3)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import levelsetfusion_python_amd as lsf  # noqa: E402
from levelsetfusion_python_amd import device_fusion, device_rigid, synthetic  # noqa: E402
from levelsetfusion_python_amd.tsdf import generation as gen  # noqa: E402

K = np.array([[700.0, 0, 320], [0, 700.0, 240], [0, 0, 1]], dtype=np.float32)
CAM = gen.DepthCamera(intrinsics=gen.DepthCamera.Intrinsics(intrinsic_matrix=K))
HBM = 8e12
TWIST = np.array([0.001, -0.001, 0.002, 0.002, -0.003, 0.001])


def case(n):
    off = np.array([-n // 2, -n // 2, 250 - n // 2])
    depth, code = gen.device_depth(synthetic.depth_image(shift_px=2.0, nearer_m=0.008))
    model = lsf.fusion.CanonicalVolume(n)
    model.integrate_depth(synthetic.depth_image(), CAM, np.zeros(6), off)
    live = device_rigid.live_volume_3d(depth, code, CAM, n, off, TWIST)
    torch.cuda.synchronize()
    return model, depth, code, live, off


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


def fuse_rows():
    rows = []
    for n in (128, 256, 512):
        model, depth, code, live, off = case(n)
        t, w = model.tsdf.clone(), model.weight.clone()
        vol_ms = best_ms(lambda: device_fusion.integrate_volume(t, w, live))
        dep_ms = best_ms(lambda: device_fusion.integrate_depth(t, w, depth, code, CAM, off, TWIST))
        rec = device_fusion.unpack_record(device_fusion.integrate_volume(t, w, live).cpu().numpy())
        image = depth.numel() * depth.element_size()
        for mode, ms, bpv, extra in (("volume", vol_ms, 20, 0), ("depth", dep_ms, 16, image)):
            moved = bpv * n ** 3 + extra
            rows.append(dict(n=n, mode=mode, device_us=ms * 1e3, bytes_per_voxel=bpv, image_bytes=extra,
                             effective_tb_s=moved / (ms * 1e-3) / 1e12, fraction_of_8tb_s=moved / (ms * 1e-3) / HBM,
                             observed_fraction=rec["fused"] / n ** 3))
            print(json.dumps(rows[-1]), flush=True)
        del model, t, w, live
        torch.cuda.empty_cache()
    return rows


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e3


def split_rows(nonrigid_iterations=10, rigid_iterations=60):
    rows = []
    for n in (128, 256):
        off = np.array([-n // 2, -n // 2, 250 - n // 2])
        d0, d1 = synthetic.depth_image(), synthetic.depth_image(shift_px=2.0, nearer_m=0.008)
        opt = lsf.SlavchevaOptimizer3d(field_size=n, compute_method=lsf.ComputeMethod.DIRECT,
                                       smoothing_term_method=lsf.SmoothingTermMethod.KILLING,
                                       level_set_term_enabled=True, maximum_warp_length_lower_threshold=0.0,
                                       max_iterations=nonrigid_iterations, min_iterations=nonrigid_iterations)
        for label, optimizer in (("rigid + fuse", None), ("rigid + non-rigid + fuse", opt)):
            best = None
            for _ in range(3):
                seq = lsf.SequenceFusion3d(CAM, n, off, rigid_iterations=rigid_iterations, nonrigid_optimizer=optimizer)
                seq.integrate(d0)
                depth, code = gen.device_depth(d1)
                model = seq.canonical
                (twist, _), rigid = timed(lambda: device_rigid.rigid_run_3d(
                    model.tsdf, depth, code, CAM, off, rigid_iterations, 0.5, 0.01, 0.004, 0.004, 20, twist=np.zeros(6)))
                if optimizer is None:
                    live_ms, nonrigid = 0.0, 0.0
                    _, fuse = timed(lambda: device_fusion.integrate_depth(model.tsdf, model.weight, depth, code, CAM,
                                                                          off, twist).cpu())
                else:
                    live, live_ms = timed(lambda: device_rigid.live_volume_3d(depth, code, CAM, n, off, twist))
                    _, nonrigid = timed(lambda: optimizer.optimize(live, model.tsdf))
                    _, fuse = timed(lambda: device_fusion.integrate_volume(model.tsdf, model.weight, live).cpu())
                _, whole = timed(lambda: seq.integrate(d1))
                row = dict(n=n, path=label, rigid_ms=rigid, live_ms=live_ms, nonrigid_ms=nonrigid, fuse_ms=fuse,
                           integrate_wall_ms=whole, nonrigid_iterations=nonrigid_iterations if optimizer else 0,
                           rigid_iterations=rigid_iterations)
                if best is None or row["integrate_wall_ms"] < best["integrate_wall_ms"]:
                    best = row
            rows.append(best)
            print(json.dumps(best), flush=True)
    return rows


def write_md(path, fuse, split):
    lines = ["# Cost of fusion into a canonical TSDF volume (MI355X)", "",
             "`tools/fusion_cost.py` (raw numbers: `fusion_cost.json`; one call of each mode at 256³ under",
             "`rocprofv3 --kernel-trace --stats`: `fusion_kernel_stats.csv`).  The synthetic frame",
             "`synthetic.depth_image(shift_px=2, nearer_m=0.008)` fused into a model that holds `depth_image()`, 4 mm "
             "voxels,", "the surface at 1 m in the middle of the volume, 20-voxel band.  Device time is one call (the "
             "fuse launch", "and the one-workgroup finishing launch), events around it, best of 10.  The byte model: "
             "volume mode reads", "live, tsdf and weight and writes tsdf and weight (20 B/voxel); depth mode does not "
             "read a live volume (16 B/voxel)", "plus the depth image.  Steps of four voxels with no observed voxel "
             "store nothing, so the model overstates the", "writes; the fraction of 8 TB/s is that of the byte model.",
             "", "| volume | mode | device / call | B / voxel | effective TB/s | of 8 TB/s | observed voxels |",
             "|---|---|---|---|---|---|---|"]
    for r in fuse:
        lines.append("| %d³ | %s | %.1f µs | %d%s | %.2f | %.0f %% | %.1f %% |" % (
            r["n"], r["mode"], r["device_us"], r["bytes_per_voxel"], " + image" if r["image_bytes"] else "",
            r["effective_tb_s"], 100 * r["fraction_of_8tb_s"], 100 * r["observed_fraction"]))
    lines += ["", "**Per-frame split** of `SequenceFusion3d.integrate` (the second frame; each step timed between "
              "device", "synchronisations, so host work is included; best of 3 by whole-frame wall time; %d rigid "
              "iterations, the" % split[0]["rigid_iterations"],
              "non-rigid step a KillingFusion-style `SlavchevaOptimizer3d`, DIRECT, %d iterations):"
              % max(r["nonrigid_iterations"] for r in split), "",
              "| volume | path | rigid | live volume | non-rigid | fuse + record read | `integrate()` wall |",
              "|---|---|---|---|---|---|---|"]
    for r in split:
        lines.append("| %d³ | %s | %.2f ms | %.2f ms | %.2f ms | %.3f ms | %.2f ms |" % (
            r["n"], r["path"], r["rigid_ms"], r["live_ms"], r["nonrigid_ms"], r["fuse_ms"], r["integrate_wall_ms"]))
    lines.append("")
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--trace":
        n = int(sys.argv[2])
        model, depth, code, live, off = case(n)
        device_fusion.integrate_volume(model.tsdf, model.weight, live)
        r = device_fusion.integrate_depth(model.tsdf, model.weight, depth, code, CAM, off, TWIST)
        print(json.dumps(dict(n=n, record=device_fusion.unpack_record(r.cpu().numpy()))))
        return
    fuse = fuse_rows()
    split = split_rows()
    stem = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "fusion_cost")
    with open(stem + ".json", "w") as f:
        json.dump(dict(fuse=fuse, frame_split=split), f, indent=1)
    write_md(stem + ".md", fuse, split)


if __name__ == "__main__":
    main()
