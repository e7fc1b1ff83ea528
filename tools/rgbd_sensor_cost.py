"""Cost of the RGB-D sensor front end (profiles/rgbd_sensor_cost.md, .json).
1. The three entry points (device_rgbd.ray_table, rectify_colour, register_depth) at two sizes -- a 640 x 480 depth
   camera into a 640 x 480 colour camera, and a 512 x 424 one into 1920 x 1080 -- with a barrel lens on the depth camera
   and five coefficients on the colour camera, the depth image fusion_scene's rendered through the depth camera's matrix.
   The figures and the timing method are tools/colour_cost.py's (queued, single, host), the calls alternating within
   every repetition.
2. A tracked and fused frame of SequenceFusion3d at 128^3 ("icp" tracking, colour) on the rig scene
   (tests/rgbd_rig_scene.py) with sensor= on the raw pairs and without it on the registered pairs: host clock around
   integrate() and a device wait, the two sequences alternating within every repetition.  The run without is the code
   that did not change.
usage: rgbd_sensor_cost.py [OUT_STEM]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import colour_cost as CC  # noqa: E402
import colour_scene as CS  # noqa: E402
import fusion_scene as S  # noqa: E402
import rgbd_restatement as G  # noqa: E402
import rgbd_rig_scene as RS  # noqa: E402
import levelsetfusion_python_amd as lsf  # noqa: E402
from levelsetfusion_python_amd import device_rgbd as D  # noqa: E402

N = 128
FRAME_REPS = 7


def matrix(f, cx, cy):
    return np.array([[f, 0, cx], [0, f, cy], [0, 0, 1.0]])


SIZES = (
    dict(name="640 x 480 into 640 x 480", depth_shape=(480, 640), depth_K=matrix(580.0, 319.5, 239.5),
         colour_shape=(480, 640), colour_K=matrix(525.0, 319.5, 239.5), transform=G.transform((0, 0.01, 0), (0.025, 0, 0))),
    dict(name="512 x 424 into 1920 x 1080", depth_shape=(424, 512), depth_K=matrix(365.0, 255.5, 211.5),
         colour_shape=(1080, 1920), colour_K=matrix(1060.0, 959.5, 539.5),
         transform=G.transform((0, 0.01, 0), (0.052, 0, 0))),
)


def entry_points(size, blocker):
    h, w = size["depth_shape"]
    ho, wo = size["colour_shape"]
    depth = torch.from_numpy(S.render(S.true_twist(0), w, h, size["depth_K"])).cuda()
    image = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (ho, wo, 3), dtype=np.uint8)).cuda()
    corner, centre = D.ray_table((h, w), size["depth_K"], G.BARREL)
    dst, valid = D.rectify_colour(image, size["colour_K"], RS.COLOUR_COEFFS, size["colour_K"], (ho, wo))
    zbuffer = torch.empty((ho, wo), dtype=torch.int32, device="cuda")
    out = torch.empty((ho, wo), dtype=torch.float32, device="cuda")
    record = torch.empty(8, dtype=torch.int64, device="cuda")
    register = lambda: D.register_depth(depth, corner, centre, size["transform"], size["colour_K"], (ho, wo), 1.0, 8,
                                        valid, zbuffer, out, record)
    fns = {"ray_table": lambda: D.ray_table((h, w), size["depth_K"], G.BARREL, corner, centre),
           "rectify_colour": lambda: D.rectify_colour(image, size["colour_K"], RS.COLOUR_COEFFS, size["colour_K"],
                                                      (ho, wo), dst, valid),
           "register_depth": register}
    kernels = CC.measure(fns, blocker)
    register()
    counts = D.unpack_record(record.cpu().numpy())
    return dict(name=size["name"], depth_pixels=h * w, output_pixels=ho * wo, record=counts, kernels=kernels)


def frames(blocker):
    """wall ms of integrate() per tracked and fused frame (k >= 1), with sensor= on the raw pairs and without it on
    the registered pairs"""
    depth_camera, colour_camera = RS.cameras()
    make_sensor = lambda: lsf.fusion.RgbdSensor(depth_camera, colour_camera, RS.DEPTH_TO_COLOUR)
    raw = [(torch.from_numpy(np.array(d)).cuda(), torch.from_numpy(np.array(c)).cuda()) for d, c in RS.raw_frames()]
    first = make_sensor()
    registered = [first.register(d, c) for d, c in raw]
    settings = dict(colour=True, colour_band=CS.COLOUR_BAND, tracking_reference="icp")
    off = CC.offset(N)
    times = {"without sensor": [], "with sensor": []}
    for rep in range(2 + FRAME_REPS):
        order = list(times) if rep % 2 == 0 else list(times)[::-1]
        for name in order:
            if name == "with sensor":
                seq = lsf.fusion.SequenceFusion3d(None, N, off, sensor=make_sensor(), **settings)
                pairs = raw
            else:
                seq = lsf.fusion.SequenceFusion3d(first.camera, N, off, **settings)
                pairs = registered
            for k, (d, c) in enumerate(pairs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                seq.integrate(d, c)
                torch.cuda.synchronize()
                if rep >= 2 and k >= 1:
                    times[name].append((time.perf_counter() - t0) * 1e3)
            del seq
    # the registration alone on a raw pair already on the card, queued: what the sensor adds on the device
    sensor = make_sensor()
    dev_pair = raw[1]
    sensor.register(*dev_pair)
    call = CC.measure({"RgbdSensor.register": lambda: sensor.register_device(*dev_pair)}, blocker)
    return dict(n=N, frames_per_sequence=len(raw), reps=FRAME_REPS, wall_ms={k: CC.stats(v) for k, v in times.items()},
                register=call["RgbdSensor.register"])


def write_md(path, sizes, frame):
    lines = ["# Cost of the RGB-D sensor front end (MI355X)", "",
             "`tools/rgbd_sensor_cost.py` (raw numbers: `rgbd_sensor_cost.json`).  Nothing here had been measured before, so no",
             "target was set in advance; the numbers are reported.", "",
             "## The entry points", "",
             "A barrel lens `k = (-0.25, 0.08, 0.001, -0.0005)` on the depth camera, five coefficients on the colour camera,",
             "`max_footprint = 8`, float32 depth in metres.  The timing method and the three figures are",
             "`tools/colour_cost.py`'s: *queued* is device time per call with the host off the critical path (%d calls" % CC.QUEUE,
             "enqueued behind several ms of other device work), *single* is HIP events around one call on an idle stream with",
             "the wrapper's checks inside the window, *host* is the host clock around the enqueue.  Medians of %d repetitions" % CC.REPS,
             "after %d warm-up calls.  `ray_table` runs once per sensor; `register_depth` is three launches (clear, splat," % CC.WARMUP,
             "finalise), the other two one each.", "",
             "| size | call | queued | single | host |", "|---|---|---|---|---|"]
    for s in sizes:
        for call, r in s["kernels"].items():
            lines.append("| %s | %s | %.1f µs | %.1f µs | %.1f µs |" % (s["name"], call, r["queued"]["median"],
                                                                         r["single"]["median"], r["host"]["median"]))
    lines += ["", "| size | depth pixels | output pixels | " + " | ".join(D.RECORD_FIELDS) + " |",
              "|---|---|---|" + "---|" * len(D.RECORD_FIELDS)]
    for s in sizes:
        lines.append("| %s | %d | %d | " % (s["name"], s["depth_pixels"], s["output_pixels"])
                     + " | ".join(str(s["record"][f]) for f in D.RECORD_FIELDS) + " |")
    w = frame["wall_ms"]
    r = frame["register"]
    lines += ["", "## A tracked and fused frame", "",
              "`SequenceFusion3d` at %d³, `tracking_reference=\"icp\"`, `colour=True`, on the rig scene" % frame["n"],
              "(`tests/rgbd_rig_scene.py`: 512 x 384 depth into 640 x 480 colour): host clock around `integrate()` and a device",
              "wait, frames k >= 1 of %d-frame sequences, %d repetitions after 2 warm-up ones, the two sequences alternating." % (frame["frames_per_sequence"], frame["reps"]),
              "*Without sensor* is fed the registered pairs and is the code that did not change; *with sensor* is fed the raw",
              "pairs; both as device tensors.", "",
              "| sequence | median | p25 | p75 | frames |", "|---|---|---|---|---|"]
    for name, v in w.items():
        lines.append("| %s | %.3f ms | %.3f ms | %.3f ms | %d |" % (name, v["median"], v["p25"], v["p75"], v["count"]))
    lines += ["", "`RgbdSensor.register` alone on a raw pair already on the card (rectify, then register: four launches): "
              "%.1f µs queued, %.1f µs single, %.1f µs of host time." % (r["queued"]["median"], r["single"]["median"],
                                                                         r["host"]["median"]), "", ""]
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    stem = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rgbd_sensor_cost")
    os.makedirs(os.path.dirname(os.path.abspath(stem)), exist_ok=True)
    assert torch.cuda.is_available(), "the cost of the sensor front end is measured on the GPU"
    blocker = torch.zeros(CC.BLOCKER_FLOATS, dtype=torch.float32, device="cuda")
    sizes = []
    for size in SIZES:
        sizes.append(entry_points(size, blocker))
        print(json.dumps(sizes[-1]), flush=True)
    frame = frames(blocker)
    print(json.dumps(frame), flush=True)
    with open(stem + ".json", "w") as f:
        json.dump(dict(sizes=sizes, frame=frame, warmup=CC.WARMUP, reps=CC.REPS, queue=CC.QUEUE), f, indent=1)
    write_md(stem + ".md", sizes, frame)


if __name__ == "__main__":
    main()
