"""Cost of projective point-to-plane ICP (profiles/icp_cost.md, .json) on the synthetic depth frames of
tools/raycast_cost.py (synthetic.depth_image, K = [[700, 0, 320], [0, 700, 240], [0, 0, 1]], 4 mm voxels, the surface
at 1 m in the middle of the volume; the second frame shifted 2 px and 8 mm nearer):
  * device time of one ICP iteration at 640 x 480 for strides 1, 2 and 4: events around device_icp.icp_run with 1 and
    with 21 iterations at one stride, (t21 - t1) / 20, best of 10 each; the prediction is the 256^3 model ray-cast with
    normals at the identity
  * one whole ProjectiveIcp3d.optimize (iterations (4, 4, 6) at strides (4, 2, 1)): device time (events) and host wall
    time, best of 10, with the spread of the 10
  * the per-frame split of SequenceFusion3d.integrate at 128^3 and 256^3 for tracking_reference "raycast" and "icp",
    in the format of profiles/raycast_cost.md (the second frame; each step timed between device synchronisations,
    best of 3 by whole-frame wall time)
usage: icp_cost.py [OUT_STEM]        icp_cost.py --trace N    (one optimize() at an N^3 model, for rocprofv3)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import levelsetfusion_python_amd as lsf  # noqa: E402
from levelsetfusion_python_amd import _lib, device_fusion, device_icp, device_raycast, device_rigid, synthetic  # noqa: E402
from levelsetfusion_python_amd.tsdf import generation as gen  # noqa: E402

K = np.array([[700.0, 0, 320], [0, 700.0, 240], [0, 0, 1]], dtype=np.float32)
CAM = gen.DepthCamera(intrinsics=gen.DepthCamera.Intrinsics(intrinsic_matrix=K))
METRIC = gen.DepthCamera(intrinsics=gen.DepthCamera.Intrinsics(intrinsic_matrix=K), depth_unit_ratio=1.0)


def offset(n):
    return np.array([-n // 2, -n // 2, 250 - n // 2])


def model(n):
    vol = lsf.fusion.CanonicalVolume(n)
    vol.integrate_depth(synthetic.depth_image(), CAM, np.zeros(6), offset(n))
    torch.cuda.synchronize()
    return vol


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def samples(fn, reps=10):
    fn()
    return [event_ms(fn) for _ in range(reps)]


def prediction(vol, n):
    depth, normals, hits = device_raycast.raycast(vol.tsdf, vol.weight, CAM, np.zeros(6), offset(n), normals=True)
    return depth, normals, int(hits.item())


def iteration_rows(pd, pn, live, code):
    rows = []
    for stride in (1, 2, 4):
        one = samples(lambda: device_icp.icp_run(live, code, pd, pn, CAM, np.zeros(6), iterations=(1,),
                                                 strides=(stride,)))
        many = samples(lambda: device_icp.icp_run(live, code, pd, pn, CAM, np.zeros(6), iterations=(21,),
                                                  strides=(stride,)))
        per = [(m - o) / 20 * 1e3 for o, m in zip(one, many)]
        _, recs, _ = device_icp.icp_run(live, code, pd, pn, CAM, np.zeros(6), iterations=(1,), strides=(stride,))
        rows.append(dict(stride=stride, iteration_us=(min(many) - min(one)) / 20 * 1e3, spread_us=[min(per), max(per)],
                         call_1_ms=min(one), call_21_ms=min(many), correspondences=int(recs[0][56]),
                         live_pixels=((480 + stride - 1) // stride) * ((640 + stride - 1) // stride)))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def optimize_row(pd, pn, d1):
    tracker = lsf.ProjectiveIcp3d(CAM)
    dev = samples(lambda: tracker.optimize(d1, pd, pn, np.zeros(6)))
    wall = []
    for _ in range(10):
        torch.cuda.synchronize()
        t = time.perf_counter()
        tracker.optimize(d1, pd, pn, np.zeros(6))
        wall.append((time.perf_counter() - t) * 1e3)
    row = dict(device_ms=min(dev), device_spread_ms=[min(dev), max(dev)], wall_ms=min(wall),
               wall_spread_ms=[min(wall), max(wall)], iterations=list(tracker.iterations),
               strides=list(tracker.strides), skipped=sum(r["skipped"] for r in tracker.last_records),
               last_count=tracker.last_records[-1]["count"])
    print(json.dumps(row), flush=True)
    return row


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
        off = offset(n)
        for mode in ("raycast", "icp"):
            best, walls = None, []
            for _ in range(3):
                seq = lsf.SequenceFusion3d(CAM, n, off, rigid_iterations=rigid_iterations, tracking_reference=mode)
                seq.integrate(d0)
                m = seq.canonical
                prev, prev_code = gen.device_depth(d0)
                depth, code = gen.device_depth(d1)
                live_ms = 0.0
                if mode == "raycast":
                    (pred, _, _), cast_ms = timed(lambda: device_raycast.raycast(
                        m.tsdf, m.weight, CAM, np.zeros(6), off, image_shape=tuple(prev.shape), fallback_depth=prev,
                        fallback_code=prev_code))
                    reference, live_ms = timed(lambda: device_rigid.live_volume_3d(
                        pred, _lib.DEPTH_F32, METRIC, (n,) * 3, off, np.zeros(6)))
                    (twist, _), track = timed(lambda: device_rigid.rigid_run_3d(
                        reference, depth, code, CAM, off, rigid_iterations, 0.5, 0.01, 0.004, 0.004, 20,
                        twist=np.zeros(6)))
                else:
                    (pred, normals, _), cast_ms = timed(lambda: device_raycast.raycast(
                        m.tsdf, m.weight, CAM, np.zeros(6), off, image_shape=tuple(depth.shape), normals=True))
                    (twist, _, _), track = timed(lambda: device_icp.icp_run(depth, code, pred, normals, CAM,
                                                                            np.zeros(6)))
                t_, w_ = m.tsdf.clone(), m.weight.clone()
                _, fuse = timed(lambda: device_fusion.integrate_depth(t_, w_, depth, code, CAM, off, twist).cpu())
                _, whole = timed(lambda: seq.integrate(d1))
                walls.append(whole)
                row = dict(n=n, tracking_reference=mode, raycast_ms=cast_ms, prediction_volume_ms=live_ms,
                           tracking_ms=track, fuse_ms=fuse, integrate_wall_ms=whole,
                           iterations=rigid_iterations if mode == "raycast" else sum(seq.icp_iterations),
                           prediction_hits=seq.frame_records[-1]["prediction_hits"])
                if best is None or row["integrate_wall_ms"] < best["integrate_wall_ms"]:
                    best = row
            best["integrate_wall_spread_ms"] = [min(walls), max(walls)]
            rows.append(best)
            print(json.dumps(best), flush=True)
    return rows


def write_md(path, it_rows, opt, split, hits):
    lines = ["# Cost of projective point-to-plane ICP (MI355X)", "",
             "`tools/icp_cost.py` (raw numbers: `icp_cost.json`; one `ProjectiveIcp3d.optimize` at 256³ under",
             "`rocprofv3 --kernel-trace --stats`: `icp_kernel_stats.csv`).  The frames are those of",
             "`profiles/raycast_cost.md`: `synthetic.depth_image()` fused into the model, the second frame (2 px to",
             "the side, 8 mm nearer) tracked.  The prediction is the 256³ model ray-cast with normals at the",
             "identity, 640 x 480 (%d hits)." % hits, "",
             "**Per iteration** at 640 x 480: events around `device_icp.icp_run` with 21 and with 1 iteration at one",
             "stride, `(t21 - t1) / 20`, best of 10 (the range of the 10 pairs in brackets):", "",
             "| stride | live pixels | correspondences | device / iteration |", "|---|---|---|---|"]
    for r in it_rows:
        lines.append("| %d | %d | %d | %.1f µs (%.1f–%.1f) |" % (r["stride"], r["live_pixels"], r["correspondences"],
                                                                  r["iteration_us"], *r["spread_us"]))
    lines += ["", "**One `ProjectiveIcp3d.optimize`** (iterations %s at strides %s: %d launches and one copy back):"
              % (tuple(opt["iterations"]), tuple(opt["strides"]), sum(opt["iterations"]) + 1),
              "device %.3f ms (%.3f–%.3f over 10), host wall %.3f ms (%.3f–%.3f)." % (
                  opt["device_ms"], *opt["device_spread_ms"], opt["wall_ms"], *opt["wall_spread_ms"]), "",
              "**Per-frame split** of `SequenceFusion3d.integrate` (the second frame; each step timed between "
              "device", "synchronisations, so host work is included; best of 3 by whole-frame wall time, the range "
              "of the 3 in", "brackets; 60 rigid iterations in \"raycast\" mode, 14 ICP iterations in \"icp\" mode, "
              "no non-rigid step):", "",
              "| volume | tracking_reference | ray-cast | prediction's live volume | tracking run | fuse + record read "
              "| `integrate()` wall |", "|---|---|---|---|---|---|---|"]
    for r in split:
        lines.append("| %d³ | %s | %.3f ms | %.3f ms | %.3f ms | %.3f ms | %.2f ms (%.2f–%.2f) |" % (
            r["n"], r["tracking_reference"], r["raycast_ms"], r["prediction_volume_ms"], r["tracking_ms"],
            r["fuse_ms"], r["integrate_wall_ms"], *r["integrate_wall_spread_ms"]))
    lines.append("")
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--trace":
        n = int(sys.argv[2])
        vol = model(n)
        pd, pn, hits = prediction(vol, n)
        twist = lsf.ProjectiveIcp3d(CAM).optimize(synthetic.depth_image(shift_px=2.0, nearer_m=0.008), pd, pn,
                                                  np.zeros(6))
        print(json.dumps(dict(n=n, hits=hits, twist=twist.tolist())))
        return
    vol = model(256)
    pd, pn, hits = prediction(vol, 256)
    d1 = synthetic.depth_image(shift_px=2.0, nearer_m=0.008)
    live, code = gen.device_depth(d1)
    it_rows = iteration_rows(pd, pn, live, code)
    opt = optimize_row(pd, pn, d1)
    del vol, pd, pn
    torch.cuda.empty_cache()
    split = split_rows()
    stem = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "icp_cost")
    with open(stem + ".json", "w") as f:
        json.dump(dict(prediction_hits=hits, iteration=it_rows, optimize=opt, frame_split=split), f, indent=1)
    write_md(stem + ".md", it_rows, opt, split, hits)


if __name__ == "__main__":
    main()
