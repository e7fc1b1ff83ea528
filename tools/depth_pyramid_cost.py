"""Cost of the live depth pyramid and of ICP over it (profiles/depth_pyramid_cost.md, .json), on the frames of
tools/icp_cost.py (synthetic.depth_image, K = [[700, 0, 320], [0, 700, 240], [0, 0, 1]], 4 mm voxels; the second frame
shifted 2 px and 8 mm nearer), 640 x 480:
  * device time of device_depth_pyramid.depth_pyramid (events, best of 10, with the range of the 10): the filter alone
    is (levels 1, radius 3) - (levels 1, radius 0); a coarser level is (levels l + 1) - (levels l), both radius 3
  * one ProjectiveIcp3d.optimize with the default DepthPyramid and a 20 degree gate (iterations (4, 4, 6)): device time
    (events) and host wall time, best of 10, with the range, next to today's strided tracker
  * the per-frame split of SequenceFusion3d.integrate in "icp" mode with and without icp_pyramid at 128^3 and 256^3
    (the second frame; each step timed between device synchronisations, best of 3 by whole-frame wall time)
usage: depth_pyramid_cost.py [OUT_STEM]    depth_pyramid_cost.py --trace N   (one pyramid optimize() at N^3, for rocprofv3)"""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import levelsetfusion_python_amd as lsf  # noqa: E402
from levelsetfusion_python_amd import device_depth_pyramid, device_fusion, device_icp, device_raycast, synthetic  # noqa: E402
from levelsetfusion_python_amd.tsdf import generation as gen  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from icp_cost import CAM, event_ms, model, offset, prediction, samples, timed  # noqa: E402

ANGLE = math.radians(20.0)


def spread(xs):
    return [min(xs), max(xs)]


def pyramid_rows(live, code):
    rows = {}
    for levels, radius in ((1, 0), (1, 3), (2, 3), (3, 3), (4, 3)):
        t = samples(lambda: device_depth_pyramid.depth_pyramid(live, code, CAM, levels=levels, radius=radius))
        rows["L%d_r%d" % (levels, radius)] = dict(levels=levels, radius=radius, launches=levels + 1,
                                                  device_ms=min(t), spread_ms=spread(t))
        print(json.dumps(rows["L%d_r%d" % (levels, radius)]), flush=True)
    return rows


def optimize_rows(pd, pn, d1):
    rows = []
    for name, kw in (("stride", {}), ("pyramid", dict(pyramid=lsf.rigid_opt.DepthPyramid())),
                     ("pyramid + gate", dict(pyramid=lsf.rigid_opt.DepthPyramid(), max_normal_angle=ANGLE))):
        tracker = lsf.ProjectiveIcp3d(CAM, **kw)
        dev = samples(lambda: tracker.optimize(d1, pd, pn, np.zeros(6)))
        wall = []
        for _ in range(10):
            torch.cuda.synchronize()
            t = time.perf_counter()
            tracker.optimize(d1, pd, pn, np.zeros(6))
            wall.append((time.perf_counter() - t) * 1e3)
        row = dict(tracker=name, device_ms=min(dev), device_spread_ms=spread(dev), wall_ms=min(wall),
                   wall_spread_ms=spread(wall), last_count=tracker.last_records[-1]["count"],
                   last_angle_rejected=tracker.last_records[-1]["angle_rejected"])
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def split_rows():
    rows = []
    d0, d1 = synthetic.depth_image(), synthetic.depth_image(shift_px=2.0, nearer_m=0.008)
    for n in (128, 256):
        off = offset(n)
        for name in ("stride", "pyramid + gate"):
            kw = {} if name == "stride" else dict(icp_pyramid=lsf.rigid_opt.DepthPyramid(), icp_max_normal_angle=ANGLE)
            best, walls = None, []
            for _ in range(3):
                seq = lsf.SequenceFusion3d(CAM, n, off, tracking_reference="icp", **kw)
                seq.integrate(d0)
                m = seq.canonical
                depth, code = gen.device_depth(d1)
                (pred, normals, _), cast_ms = timed(lambda: device_raycast.raycast(
                    m.tsdf, m.weight, CAM, np.zeros(6), off, image_shape=tuple(depth.shape), normals=True))
                pyr_ms = 0.0
                if name == "stride":
                    (twist, _, _), track = timed(lambda: device_icp.icp_run(depth, code, pred, normals, CAM,
                                                                            np.zeros(6)))
                else:
                    levels, pyr_ms = timed(lambda: seq.icp_pyramid.build(depth, CAM))
                    (twist, _, _), track = timed(lambda: device_icp.icp_run_pyramid(
                        *levels.buffers, 3, pred, normals, CAM, np.zeros(6), max_normal_angle=ANGLE))
                t_, w_ = m.tsdf.clone(), m.weight.clone()
                _, fuse = timed(lambda: device_fusion.integrate_depth(t_, w_, depth, code, CAM, off, twist).cpu())
                _, whole = timed(lambda: seq.integrate(d1))
                walls.append(whole)
                row = dict(n=n, tracker=name, raycast_ms=cast_ms, pyramid_ms=pyr_ms, tracking_ms=track,
                           fuse_ms=fuse, integrate_wall_ms=whole)
                if best is None or row["integrate_wall_ms"] < best["integrate_wall_ms"]:
                    best = row
            best["integrate_wall_spread_ms"] = spread(walls)
            rows.append(best)
            print(json.dumps(best), flush=True)
    return rows


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--trace":
        n = int(sys.argv[2])
        vol = model(n)
        pd, pn, hits = prediction(vol, n)
        tracker = lsf.ProjectiveIcp3d(CAM, pyramid=lsf.rigid_opt.DepthPyramid(), max_normal_angle=ANGLE)
        twist = tracker.optimize(synthetic.depth_image(shift_px=2.0, nearer_m=0.008), pd, pn, np.zeros(6))
        print(json.dumps(dict(n=n, hits=hits, twist=twist.tolist())))
        return
    vol = model(256)
    pd, pn, hits = prediction(vol, 256)
    d1 = synthetic.depth_image(shift_px=2.0, nearer_m=0.008)
    live, code = gen.device_depth(d1)
    pyr = pyramid_rows(live, code)
    opt = optimize_rows(pd, pn, d1)
    del vol, pd, pn
    torch.cuda.empty_cache()
    split = split_rows()
    stem = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "depth_pyramid_cost")
    with open(stem + ".json", "w") as f:
        json.dump(dict(prediction_hits=hits, pyramid=pyr, optimize=opt, frame_split=split), f, indent=1)


if __name__ == "__main__":
    main()
