"""Cost of colour fusion next to weighted fusion in the same build (profiles/colour_cost.md, .json), on the analytic sphere
scene of the tests (tests/colour_scene.py: three spheres and a plane, K = [[700, 0, 320], [0, 700, 240], [0, 0, 1]],
640 x 480, 4 mm voxels, 20-voxel band), at 128^3 and 256^3, on a model that already holds frame 0.  Three figures per
entry point, device_fusion.integrate_depth_weighted and device_fusion.integrate_depth_colour with the same arguments,
the two alternating within every repetition:
  queued  device time per call with the host off the critical path: QUEUE calls enqueued behind a long elementwise
          launch, HIP events around them; a repetition counts only if the host had enqueued everything before the
          device got there (both launches of each call, and the gaps between launches)
  single  HIP events around one call on an idle stream: the Python wrapper's argument checks run inside this window
  host    host clock around the enqueue of one call (no device wait): the wrapper alone
The kernels' own times come from `rocprofv3 --kernel-trace --stats -- python colour_cost.py --trace N`, a run of its own.
usage: colour_cost.py [OUT_STEM]        colour_cost.py --trace N    (ten calls of each kind, for rocprofv3)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import colour_scene as CS  # noqa: E402
import fusion_scene as S  # noqa: E402
import levelsetfusion_python_amd as lsf  # noqa: E402
from levelsetfusion_python_amd import device_fusion  # noqa: E402
from levelsetfusion_python_amd.tsdf import generation as gen  # noqa: E402

CAM = gen.DepthCamera(intrinsics=gen.DepthCamera.Intrinsics(intrinsic_matrix=S.K), depth_unit_ratio=1.0)
WARMUP, REPS, QUEUE = 5, 30, 16
BLOCKER_FLOATS, BLOCKER_LAUNCHES = 1 << 29, 8  # 2 GiB read and written eight times: several ms of device work


def offset(n):
    """the volume around the spheres and the plane: fusion_scene.offset's placement at any n"""
    return np.array([-n / 2, -n / 2, 0.53 / 0.004 - n / 2], dtype=np.float64)


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def single_us(fn):
    """device time between events around one call on an idle stream; the wrapper's host work is inside the window"""
    a, b = events()
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3


def queued_us(fn, blocker):
    """(device us per call, host us per call, queued ahead): QUEUE calls enqueued while the device works on the blocker;
    queued ahead says that the host was done before the blocker was, so no host work lies between the events"""
    z, (a, b) = torch.cuda.Event(enable_timing=True), events()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    z.record()
    for _ in range(BLOCKER_LAUNCHES):
        blocker.add_(1.0)
    a.record()
    t1 = time.perf_counter()
    for _ in range(QUEUE):
        fn()
    t2 = time.perf_counter()
    b.record()
    host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / QUEUE, (t2 - t1) * 1e6 / QUEUE, host_ms < z.elapsed_time(a)


def stats(x):
    return dict(median=float(np.median(x)), min=float(np.min(x)), p25=float(np.percentile(x, 25)),
                p75=float(np.percentile(x, 75)), count=len(x))


def measure(fns, blocker):
    """{name: {queued, single, host}} of the named calls, alternating them within every repetition and swapping the
    order between repetitions"""
    names = list(fns)
    for _ in range(WARMUP):
        for name in names:
            fns[name]()
    raw = {name: dict(queued=[], single=[], host=[]) for name in names}
    for rep in range(REPS):
        for name in (names if rep % 2 == 0 else names[::-1]):
            raw[name]["single"].append(single_us(fns[name]))
        for name in (names if rep % 2 == 0 else names[::-1]):
            dev, host, ahead = queued_us(fns[name], blocker)
            raw[name]["host"].append(host)
            if ahead:
                raw[name]["queued"].append(dev)
    for name in names:
        if len(raw[name]["queued"]) < REPS // 2:
            raise RuntimeError("%s: the host kept ahead of the device in only %d of %d repetitions"
                               % (name, len(raw[name]["queued"]), REPS))
    return {name: {k: stats(v) for k, v in raw[name].items()} for name in names}


def calls(n, carve, band):
    """the two calls at n^3 on a model that holds frame 0, and the colour call's record"""
    (d0, i0, _), (d1, i1, _) = CS.frames()[:2]
    off = offset(n)
    depth, code = gen.device_depth(d1)
    image = torch.from_numpy(i1.copy()).cuda()
    vol = lsf.fusion.CanonicalVolume(n, colour=True)
    vol.integrate_depth(d0, CAM, S.true_twist(0), off, colour_image=i0, carve=carve, colour_band=band)
    t, w, c = vol.tsdf.clone(), vol.weight.clone(), vol.colour.clone()
    fns = dict(
        weighted=lambda: device_fusion.integrate_depth_weighted(t, w, depth, code, CAM, off, S.true_twist(1), carve=carve),
        colour=lambda: device_fusion.integrate_depth_colour(t, w, c, depth, code, CAM, off, S.true_twist(1), image,
                                                            colour_band=band, carve=carve))
    return fns, lambda: device_fusion.unpack_colour_record(fns["colour"]().cpu().numpy())


def rows():
    out = []
    blocker = torch.zeros(BLOCKER_FLOATS, dtype=torch.float32, device="cuda")
    for n in (128, 256):
        for carve in (False, True):
            for band in (1.0, 0.25):
                fns, record = calls(n, carve, band)
                m = measure(fns, blocker)
                rec = record()
                touched = rec["fused"] + rec["carved"]
                out.append(dict(n=n, carve=carve, colour_band=band, weighted=m["weighted"], colour=m["colour"],
                                ratio=m["colour"]["queued"]["median"] / m["weighted"]["queued"]["median"],
                                updated_fraction=touched / n ** 3, coloured_fraction=rec["coloured"] / n ** 3,
                                extra_bytes=35 * rec["coloured"]))
                print(json.dumps(out[-1]), flush=True)
                del fns, record
        torch.cuda.empty_cache()
    return out


def trace(n):
    """ten calls of each kind at n^3 (carve off, colour_band 1), alternating, for a kernel trace"""
    fns, _ = calls(n, False, 1.0)
    for _ in range(10):
        fns["weighted"]()
        fns["colour"]()
    torch.cuda.synchronize()


def write_md(path, table):
    def spread(m):
        return max(r[k][m]["p75"] - r[k][m]["p25"] for r in table for k in ("weighted", "colour"))

    lines = ["# Cost of colour fusion next to weighted fusion (MI355X)", "",
             "`tools/colour_cost.py` (raw numbers: `colour_cost.json`; kernel times of ten calls of each kind under",
             "`rocprofv3 --kernel-trace --stats`, a run of its own per size: `colour_kernel_stats_128.csv`, `_256.csv`).",
             "Frame 1 of the painted sphere scene (`tests/colour_scene.py`) fused at its true twist into a model that holds",
             "frame 0; 4 mm voxels, 20-voxel band.  Both entry points run in the same build with the same arguments and",
             "alternate within each of the %d repetitions after %d warm-up calls; every figure is a median.  The widest" %
             (REPS, WARMUP),
             "interquartile range is %.1f µs among the queued figures, %.1f µs among the single-call ones and %.1f µs among" %
             (spread("queued"), spread("single"), spread("host")),
             "the host ones.", "",
             "- *queued* is device time per call with the host off the critical path: %d calls enqueued behind several ms" % QUEUE,
             "  of other device work, HIP events around them, counted only when the host had finished enqueueing before the",
             "  device reached the first event.  It covers the fuse launch, the one-workgroup finishing launch and the gaps",
             "  between launches.",
             "- *single* is HIP events around one call on an idle stream, so the Python wrapper's argument checks run inside",
             "  the window.",
             "- *host* is the host clock around enqueueing one call, with no device wait: the wrapper alone.", "",
             "The colour call's extra traffic per coloured voxel is one 16-byte load, one 16-byte store and three image",
             "bytes (35 B); `extra bytes` is that times the coloured voxels.", "",
             "| volume | carve | colour_band | queued: weighted | colour | ratio | single: weighted | colour | host: weighted | colour "
             "| updated voxels | coloured voxels | extra bytes |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in table:
        w, c = r["weighted"], r["colour"]
        lines.append("| %d³ | %s | %.2f | %.1f µs | %.1f µs | %.2f | %.1f µs | %.1f µs | %.1f µs | %.1f µs | %.1f %% | %.2f %% "
                     "| %.2f MB |" % (r["n"], "on" if r["carve"] else "off", r["colour_band"], w["queued"]["median"],
                                      c["queued"]["median"], r["ratio"], w["single"]["median"], c["single"]["median"],
                                      w["host"]["median"], c["host"]["median"], 100 * r["updated_fraction"],
                                      100 * r["coloured_fraction"], r["extra_bytes"] / 1e6))
    lines += ["", ""]
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--trace":
        return trace(int(sys.argv[2]))
    table = rows()
    stem = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "colour_cost")
    os.makedirs(os.path.dirname(os.path.abspath(stem)), exist_ok=True)
    with open(stem + ".json", "w") as f:
        json.dump(dict(rows=table, warmup=WARMUP, reps=REPS, queue=QUEUE), f, indent=1)
    write_md(stem + ".md", table)


if __name__ == "__main__":
    main()
