"""Cost of the intensity pyramids and of the joint geometric and photometric ICP over the depth pyramid
(profiles/pyramid_photometric_cost.md, .json), on the frames of tools/photometric_cost.py (synthetic.depth_image,
K = [[700, 0, 320], [0, 700, 240], [0, 0, 1]], 4 mm voxels, 256^3, 640 x 480; the second frame shifted 2 px and 8 mm
nearer; a colour image painted by pixel position).  Every row has the device time between HIP events and the host's
wall-clock time of the same calls (perf_counter around the call and a synchronize), best of REPS with the range of the
REPS:
  * the builds: the depth pyramid, the live intensity pyramid, the prediction's intensity pyramid (three levels)
  * one tracking run, iterations (4, 4, 6), with the 20 degree gate and without: device_icp.icp_run_pyramid and
    icp_run_pyramid_photometric on the same pyramids and prediction
  * a tracked frame of SequenceFusion3d("icp", icp_pyramid=): the ray-cast, the pyramids and the run of one frame
    (SequenceFusion3d's own tracking step on a model that holds frame 0), without the term and with it
  * with --resources FILE (hipcc -Rpass-analysis=kernel-resource-usage of csrc/lsf_icp.hip and
    csrc/lsf_intensity_pyramid.hip): the compiler's registers, spills and scratch per kernel instantiation
usage: pyramid_photometric_cost.py [--resources FILE] [OUT_STEM]"""
import json
import math
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from photometric_cost import colour_image, load, offset  # noqa: E402

REPS, N, LAMBDA, LEVELS, GATE = 20, 256, 0.1, 3, math.radians(20.0)


def samples(torch, fn, reps=REPS):
    """(device ms between HIP events, host ms of the call and the wait for it) per repeat, after one warm-up call"""
    fn()
    device, host = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
        device.append(a.elapsed_time(b))
    return device, host


def stat(pair):
    device, host = pair
    return dict(device_ms=min(device), device_spread_ms=[min(device), max(device)], host_ms=min(host),
                host_spread_ms=[min(host), max(host)])


def measure():
    np, torch, lsf, device_icp, device_raycast, synthetic, gen, cam = load(ROOT)
    from levelsetfusion_python_amd.rigid_opt import DepthPyramid, IntensityPyramid
    off, zero = offset(np, N), np.zeros(6)
    first, first_image = synthetic.depth_image(), colour_image(np)
    vol = lsf.fusion.CanonicalVolume(N, colour=True)
    vol.integrate_depth(first, cam, zero, off, colour_image=first_image, colour_band=0.25)
    live, code = gen.device_depth(synthetic.depth_image(shift_px=2.0, nearer_m=0.008))
    image = torch.from_numpy(colour_image(np, 2.0)).cuda()
    pd, pn, hits, pc = device_raycast.raycast(vol.tsdf, vol.weight, cam, zero, off, normals=True, colour=vol.colour)
    depth_pyramid, intensity_pyramid = DepthPyramid(levels=LEVELS), IntensityPyramid(LEVELS)
    pyr = depth_pyramid.build_device(live, code, cam)
    il, ip = intensity_pyramid.build_device(image), intensity_pyramid.build_prediction(pc)

    def run(photo, gate):
        if photo:
            return device_icp.icp_run_pyramid_photometric(*pyr.buffers, il.buffer, LEVELS, pd, pn, ip.buffer, cam,
                                                          zero, LAMBDA, max_normal_angle=gate)
        return device_icp.icp_run_pyramid(*pyr.buffers, LEVELS, pd, pn, cam, zero, max_normal_angle=gate)

    def sequence(photo):
        seq = lsf.SequenceFusion3d(cam, N, off, colour=True, colour_band=0.25, tracking_reference="icp",
                                   icp_pyramid=depth_pyramid, icp_max_normal_angle=GATE,
                                   photometric_weight=LAMBDA if photo else None,
                                   icp_intensity_pyramid=intensity_pyramid if photo else None)
        seq.integrate(first, first_image)
        return lambda: seq._track_icp(live, code, zero, image if photo else None)

    out = dict(prediction_hits=int(hits.item()), prediction_coloured=int(torch.isfinite(pc[..., 3]).sum().item()),
               rows={})
    rows = [("depth_pyramid", lambda: depth_pyramid.build_device(live, code, cam)),
            ("intensity_pyramid_live", lambda: intensity_pyramid.build_device(image)),
            ("intensity_pyramid_prediction", lambda: intensity_pyramid.build_prediction(pc)),
            ("both_intensity_pyramids", lambda: (intensity_pyramid.build_device(image),
                                                 intensity_pyramid.build_prediction(pc))),
            ("run_pyramid_gate", lambda: run(False, GATE)), ("run_pyramid_photometric_gate", lambda: run(True, GATE)),
            ("run_pyramid", lambda: run(False, None)), ("run_pyramid_photometric", lambda: run(True, None)),
            ("frame", sequence(False)), ("frame_photometric", sequence(True))]
    for name, fn in rows:
        out["rows"][name] = stat(samples(torch, fn))
        print(name, json.dumps(out["rows"][name]), flush=True)
    out["last_records"] = {}
    for name, gate in (("gate", GATE), ("no_gate", None)):
        recs = [device_icp.unpack_record(r) for r in run(True, gate)[1]]
        out["last_records"][name] = dict(count=recs[-1]["count"], photometric_count=recs[-1]["photometric_count"],
                                         angle_rejected=recs[-1]["angle_rejected"],
                                         skipped=sum(r["skipped"] for r in recs))
    return out


def resources(path):
    """[(kernel, VGPRs, AGPRs, SGPR spills, VGPR spills, scratch bytes per lane, waves per SIMD)] of a
    -Rpass-analysis=kernel-resource-usage log"""
    keys = ("VGPRs", "AGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]")
    rows, name, fields = [], None, {}
    for line in open(path):
        m = re.search(r"remark:\s+(Function Name|%s): (\S+)" % "|".join(re.escape(k) for k in keys), line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = subprocess.run(["c++filt", m.group(2)], capture_output=True, text=True).stdout.strip() or m.group(2)
            name = re.sub(r"\(anonymous namespace\)::", "", name).split("(")[0].replace("void ", "")
            fields = {}
        else:
            fields[m.group(1)] = int(m.group(2))
            if len(fields) == len(keys):
                rows.append((name,) + tuple(fields[k] for k in keys))
    return rows


def write_md(path, out):
    r = out["rows"]

    def dev(k):
        return "%.3f ms (%.3f–%.3f)" % (r[k]["device_ms"], *r[k]["device_spread_ms"])

    def host(k):
        return "%.3f ms (%.3f–%.3f)" % (r[k]["host_ms"], *r[k]["host_spread_ms"])

    lines = ["# Cost of the intensity pyramids and of photometric ICP on the depth pyramid (MI355X)", "",
             "`tools/pyramid_photometric_cost.py` (raw numbers: `pyramid_photometric_cost.json`), one GPU call.  The",
             "frames are those of `profiles/photometric_cost.md`: `synthetic.depth_image()` fused into a %d³ model" % N,
             "with colour (`colour_band` 0.25), the second frame (2 px to the side, 8 mm nearer) tracked against the",
             "model ray-cast at the identity, 640 x 480 (%d hits, %d of them with a colour).  Three levels, the"
             % (out["prediction_hits"], out["prediction_coloured"]),
             "default `DepthPyramid`, iterations (4, 4, 6), λ = %g.  Device time is the time between HIP events" % LAMBDA,
             "around the calls; host time is the wall clock around the same calls and the wait for them, so it",
             "contains the device time.  Best of %d, the range of the %d in brackets." % (REPS, REPS), "",
             "| build (enqueued, no host wait inside) | device | host |", "|---|---|---|",
             "| depth pyramid (4 launches) | %s | %s |" % (dev("depth_pyramid"), host("depth_pyramid")),
             "| live intensity pyramid (3 launches) | %s | %s |" % (dev("intensity_pyramid_live"),
                                                                    host("intensity_pyramid_live")),
             "| prediction intensity pyramid (3 launches) | %s | %s |" % (dev("intensity_pyramid_prediction"),
                                                                          host("intensity_pyramid_prediction")),
             "| both intensity pyramids | %s | %s |" % (dev("both_intensity_pyramids"),
                                                        host("both_intensity_pyramids")), "",
             "| 15 launches and one copy back | `icp_run_pyramid` device | host | `icp_run_pyramid_photometric` device "
             "| host |", "|---|---|---|---|---|",
             "| tracking run, 20° gate | %s | %s | %s | %s |" % (dev("run_pyramid_gate"), host("run_pyramid_gate"),
                                                                 dev("run_pyramid_photometric_gate"),
                                                                 host("run_pyramid_photometric_gate")),
             "| tracking run, no gate | %s | %s | %s | %s |" % (dev("run_pyramid"), host("run_pyramid"),
                                                                dev("run_pyramid_photometric"),
                                                                host("run_pyramid_photometric")), "",
             "| `SequenceFusion3d` tracking step of one frame, 20° gate | device | host |", "|---|---|---|",
             "| ray-cast with normals, depth pyramid, run | %s | %s |" % (dev("frame"), host("frame")),
             "| ray-cast with normals and colour, three pyramids, joint run | %s | %s |" % (dev("frame_photometric"),
                                                                                          host("frame_photometric")),
             ""]
    for name, label in (("gate", "with the gate"), ("no_gate", "without the gate")):
        q = out["last_records"][name]
        lines.append("The last record of the joint run %s: %d geometric pairs, %d of them with a photometric term, %d "
                     "pairs rejected by the gate, %d iterations skipped." % (label, q["count"], q["photometric_count"],
                                                                            q["angle_rejected"], q["skipped"]))
    lines.append("")
    if "resources" in out:
        lines += ["**Compiler resources** (`hipcc -Rpass-analysis=kernel-resource-usage`, gfx950, 256 lanes per workgroup):",
                  "", "| kernel | VGPRs | AGPRs | SGPR spills | VGPR spills | scratch, bytes / lane | waves / SIMD |",
                  "|---|---|---|---|---|---|---|"]
        for row in out["resources"]:
            lines.append("| `%s` | %d | %d | %d | %d | %d | %d |" % row)
        new = {row[0]: row for row in out["resources"] if "PyramidPhotometricSource" in row[0]}
        gated = next((v for k, v in new.items() if "<true>" in k), None)
        plain = next((v for k, v in new.items() if "<false>" in k), None)
        if gated and plain:
            lines += ["", "No instantiation spills a vector register to memory: the scratch of every ICP row is the %d bytes"
                      % plain[5],
                      "per lane of the prologue's 6 x 6 solve on one thread, which the finishing kernel has too.  The",
                      "joint pyramid source without the gate takes %d VGPRs and keeps two waves per SIMD, like the strided"
                      % plain[1],
                      "photometric source.  With the gate it does not fit: it takes all %d VGPRs, parks values in %d"
                      % (gated[1], gated[2]),
                      "AGPRs (the other half of the register file: copies between registers, no memory traffic) and",
                      "moves %d scalar registers into lanes of a vector register (SGPR spills, again register to"
                      % gated[3],
                      "register).  That leaves one wave per SIMD, where `PyramidSource<true>` already is.  What it costs",
                      "is in the run rows above: the gated joint run against the ungated one."]
        lines.append("")
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    args = sys.argv[1:]
    res = None
    if args[:1] == ["--resources"]:
        res, args = args[1], args[2:]
    stem = args[0] if args else os.path.join(ROOT, "profiles", "pyramid_photometric_cost")
    out = measure()
    if res:
        out["resources"] = [row for row in resources(res) if "icp_iterate" in row[0] or "_kernel" in row[0] and
                            "icp_finish" not in row[0]]
    with open(stem + ".json", "w") as f:
        json.dump(out, f, indent=1)
    write_md(stem + ".md", out)


if __name__ == "__main__":
    main()
