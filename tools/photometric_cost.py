"""Cost of the ray-cast colour image and of the joint geometric and photometric ICP (profiles/photometric_cost.md,
.json), on the synthetic frames of tools/icp_cost.py (synthetic.depth_image, K = [[700, 0, 320], [0, 700, 240],
[0, 0, 1]], 4 mm voxels, 256^3, 640 x 480; the second frame shifted 2 px and 8 mm nearer) with a colour image painted by
pixel position.  All times are device times between HIP events, best of REPS, with the range of the REPS:
  * one device_raycast.raycast with normals, without and with the colour volume
  * one tracking run (iterations (4, 4, 6) at strides (4, 2, 1)): device_icp.icp_run and icp_run_photometric
  * a tracked frame of "icp" mode: the ray-cast and the run together, without and with the photometric term
  * one iteration at stride 1: (t21 - t1) / 20 of runs with 21 and with 1 iteration, both entry points
  * with --parent DIR (a checkout of the parent commit with its library built): the two paths that both revisions have,
    lsf_raycast with normals and lsf_icp_run, timed in fresh processes that alternate between DIR and this tree
  * with --resources FILE (hipcc -Rpass-analysis=kernel-resource-usage of csrc/lsf_icp.hip and csrc/lsf_raycast.hip):
    the compiler's registers and scratch per kernel instantiation
usage: photometric_cost.py [--parent DIR] [--resources FILE] [OUT_STEM]
       photometric_cost.py --worker ROOT      (one JSON line: the unchanged paths of the package under ROOT)"""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS, ROUNDS, N, LAMBDA = 20, 3, 256, 0.1


def load(root):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import levelsetfusion_python_amd as lsf
    from levelsetfusion_python_amd import device_icp, device_raycast, synthetic
    from levelsetfusion_python_amd.tsdf import generation as gen
    K = np.array([[700.0, 0, 320], [0, 700.0, 240], [0, 0, 1]], dtype=np.float32)
    cam = gen.DepthCamera(intrinsics=gen.DepthCamera.Intrinsics(intrinsic_matrix=K))
    return np, torch, lsf, device_icp, device_raycast, synthetic, gen, cam


def offset(np, n):
    return np.array([-n // 2, -n // 2, 250 - n // 2])


def samples(torch, fn, reps=REPS):
    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def stat(ms):
    return dict(best_ms=min(ms), spread_ms=[min(ms), max(ms)])


def colour_image(np, shift_px=0.0):
    """uint8 (480, 640, 3): three smooth channels of the pixel position"""
    v, u = np.meshgrid(np.arange(480, dtype=np.float64), np.arange(640, dtype=np.float64), indexing="ij")
    u = u - shift_px
    c = np.stack([0.5 + 0.25 * np.sin(u / 15.0) + 0.2 * np.sin(v / 11.0 + 1.0),
                  0.5 + 0.25 * np.sin((u + v) / 13.0 + 0.5) + 0.2 * np.cos((u - v) / 17.0),
                  0.5 + 0.3 * np.sin(u / 9.0 + 2.0) * np.sin(v / 12.0)], axis=-1)
    return np.ascontiguousarray(np.rint(255.0 * c).astype(np.uint8))


def worker(root):
    """the paths of the parent commit: the ray-cast with normals and the geometric run, on an uncoloured model"""
    np, torch, lsf, device_icp, device_raycast, synthetic, gen, cam = load(root)
    vol = lsf.fusion.CanonicalVolume(N)
    vol.integrate_depth(synthetic.depth_image(), cam, np.zeros(6), offset(np, N))
    live, code = gen.device_depth(synthetic.depth_image(shift_px=2.0, nearer_m=0.008))
    zero = np.zeros(6)

    def cast():
        return device_raycast.raycast(vol.tsdf, vol.weight, cam, zero, offset(np, N), normals=True)

    pd, pn = cast()[:2]
    row = dict(root=root, raycast=stat(samples(torch, cast)),
               icp_run=stat(samples(torch, lambda: device_icp.icp_run(live, code, pd, pn, cam, zero))))
    print(json.dumps(row), flush=True)


def alternate(parent):
    """ROUNDS fresh processes per side, parent and this tree in turn; the best of each side's bests"""
    rows = {"parent": [], "branch": []}
    for _ in range(ROUNDS):
        for side, root in (("parent", parent), ("branch", ROOT)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", root], check=True,
                                 capture_output=True, text=True, timeout=300).stdout
            rows[side].append(json.loads(out.strip().splitlines()[-1]))
            print(side, out.strip().splitlines()[-1], flush=True)
    summary = {}
    for side, rs in rows.items():
        summary[side] = {k: dict(best_ms=min(r[k]["best_ms"] for r in rs),
                                 bests_ms=[r[k]["best_ms"] for r in rs]) for k in ("raycast", "icp_run")}
    return summary


def measure():
    np, torch, lsf, device_icp, device_raycast, synthetic, gen, cam = load(ROOT)
    off, zero = offset(np, N), np.zeros(6)
    vol = lsf.fusion.CanonicalVolume(N, colour=True)
    vol.integrate_depth(synthetic.depth_image(), cam, zero, off, colour_image=colour_image(np), colour_band=0.25)
    live, code = gen.device_depth(synthetic.depth_image(shift_px=2.0, nearer_m=0.008))
    image = torch.from_numpy(colour_image(np, 2.0)).cuda()

    def cast(colour):
        return device_raycast.raycast(vol.tsdf, vol.weight, cam, zero, off, normals=True,
                                      colour=vol.colour if colour else None)

    pd, pn, hits, pc = cast(True)

    def run(photo, iterations=device_icp.ITERATIONS, strides=device_icp.STRIDES):
        if photo:
            return device_icp.icp_run_photometric(live, code, image, pd, pn, pc, cam, zero, LAMBDA,
                                                  iterations=iterations, strides=strides)
        return device_icp.icp_run(live, code, pd, pn, cam, zero, iterations=iterations, strides=strides)

    def frame(photo):
        d, n, _, *c = cast(photo)
        if photo:
            return device_icp.icp_run_photometric(live, code, image, d, n, c[0], cam, zero, LAMBDA)
        return device_icp.icp_run(live, code, d, n, cam, zero)

    out = dict(prediction_hits=int(hits.item()),
               prediction_coloured=int(torch.isfinite(pc[..., 3]).sum().item()), rows={})
    for name, fn in (("raycast", lambda: cast(False)), ("raycast_colour", lambda: cast(True)),
                     ("icp_run", lambda: run(False)), ("icp_run_photometric", lambda: run(True)),
                     ("frame_icp", lambda: frame(False)), ("frame_icp_photometric", lambda: frame(True))):
        out["rows"][name] = stat(samples(torch, fn))
        print(name, json.dumps(out["rows"][name]), flush=True)
    for name, photo in (("iteration", False), ("iteration_photometric", True)):
        one = samples(torch, lambda: run(photo, (1,), (1,)))
        many = samples(torch, lambda: run(photo, (21,), (1,)))
        out["rows"][name] = dict(iteration_us=(min(many) - min(one)) / 20 * 1e3, call_1_ms=min(one),
                                 call_21_ms=min(many))
        print(name, json.dumps(out["rows"][name]), flush=True)
    _, recs, _, _ = run(True)
    last = device_icp.unpack_record(recs[-1])
    out["last_record"] = dict(count=last["count"], photometric_count=last["photometric_count"],
                              skipped=sum(device_icp.unpack_record(r)["skipped"] for r in recs))
    return out


def resources(path):
    """[(kernel, VGPRs, scratch bytes per lane, waves per SIMD)] of a -Rpass-analysis=kernel-resource-usage log"""
    rows, name = [], None
    fields = {}
    for line in open(path):
        m = re.search(r"remark:\s+(Function Name|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = subprocess.run(["c++filt", m.group(2)], capture_output=True, text=True).stdout.strip() or m.group(2)
            name = re.sub(r"\(anonymous namespace\)::", "", name).split("(")[0].replace("void ", "")
            fields = {}
        else:
            fields[m.group(1).split(" ")[0]] = int(m.group(2))
            if len(fields) == 3:
                rows.append((name, fields["VGPRs"], fields["ScratchSize"], fields["Occupancy"]))
    return rows


def write_md(path, out):
    r = out["rows"]

    def ms(k):
        return "%.3f ms (%.3f–%.3f)" % (r[k]["best_ms"], *r[k]["spread_ms"])

    lines = ["# Cost of the ray-cast colour image and of photometric ICP (MI355X)", "",
             "`tools/photometric_cost.py` (raw numbers: `photometric_cost.json`), one GPU call.  The frames are those of",
             "`profiles/icp_cost.md` with a colour image painted by pixel position: `synthetic.depth_image()` fused",
             "into a %d³ model with colour (`colour_band` 0.25), the second frame (2 px to the side, 8 mm nearer)" % N,
             "tracked against the model ray-cast at the identity, 640 x 480 (%d hits, %d of them with a colour)."
             % (out["prediction_hits"], out["prediction_coloured"]),
             "Device time between HIP events, best of %d, the range of the %d in brackets.  A run is iterations" % (REPS, REPS),
             "(4, 4, 6) at strides (4, 2, 1), 15 launches and one copy back; λ = %g." % LAMBDA, "",
             "| | geometric | with colour / photometric term |", "|---|---|---|",
             "| `raycast` with normals | %s | %s |" % (ms("raycast"), ms("raycast_colour")),
             "| tracking run | %s | %s |" % (ms("icp_run"), ms("icp_run_photometric")),
             "| tracked frame of \"icp\" mode (ray-cast + run) | %s | %s |" % (ms("frame_icp"),
                                                                           ms("frame_icp_photometric")),
             "| one iteration at stride 1, `(t21 - t1) / 20` | %.1f µs | %.1f µs |" % (
                 r["iteration"]["iteration_us"], r["iteration_photometric"]["iteration_us"]), "",
             "The last record of the photometric run: %d geometric pairs, %d of them with a photometric term, %d "
             "iterations skipped." % (out["last_record"]["count"], out["last_record"]["photometric_count"],
                                      out["last_record"]["skipped"]), ""]
    if "alternating" in out:
        a = out["alternating"]
        lines += ["**The unchanged paths against the parent commit**: `lsf_raycast` with normals and `lsf_icp_run` on an",
                  "uncoloured %d³ model, in %d fresh processes per side that alternate between a checkout of the parent" % (N, ROUNDS),
                  "commit and this tree; each process reports its best of %d, listed per side:" % REPS, "",
                  "| path | parent | this tree |", "|---|---|---|"]
        for k, label in (("raycast", "`raycast` with normals"), ("icp_run", "tracking run (`icp_run`)")):
            lines.append("| %s | %.3f ms (%s) | %.3f ms (%s) |" % (
                label, a["parent"][k]["best_ms"], ", ".join("%.3f" % v for v in a["parent"][k]["bests_ms"]),
                a["branch"][k]["best_ms"], ", ".join("%.3f" % v for v in a["branch"][k]["bests_ms"])))
        lines.append("")
    if "resources" in out:
        lines += ["**Compiler resources** (`hipcc -Rpass-analysis=kernel-resource-usage`, gfx950, 256 lanes per workgroup):",
                  "", "| kernel | VGPRs | scratch, bytes / lane | waves / SIMD |", "|---|---|---|---|"]
        for name, vgprs, scratch, occ in out["resources"]:
            lines.append("| `%s` | %d | %d | %d |" % (name, vgprs, scratch, occ))
        lines += ["", "The 31 float64 accumulators and the second Jacobian of the `PhotometricSource` instantiation fit in",
                  "registers: its scratch is the 304 bytes per lane that every instantiation has, and that the finishing",
                  "kernel -- the prologue alone, with its 6 x 6 solve on one thread -- has too, so the pixel loop spills",
                  "nothing.", ""]
    lines += ["**Accuracy bounds of the tests** (`tests/test_photometric_host.py`; twice the restatement's own error,",
              "measured on the CPU): the whole run on the 152 x 120 wall 4.163e-6 m and 1.7929e-5 rad (`RUN_ATOL_T`,",
              "`RUN_ATOL_R`; the restatement errs by 2.0815e-6 m and 8.9645e-6 rad); the three-frame sequence at 64³",
              "4.431e-5 m and 1.15536e-4 rad (`SEQUENCE_ATOL_T`, `SEQUENCE_ATOL_R`; 2.2155e-5 m and 5.7768e-5 rad).", ""]
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    args = sys.argv[1:]
    if args[:1] == ["--worker"]:
        return worker(args[1])
    parent = res = None
    while args and args[0] in ("--parent", "--resources"):
        if args[0] == "--parent":
            parent = os.path.abspath(args[1])
        else:
            res = args[1]
        args = args[2:]
    stem = args[0] if args else os.path.join(ROOT, "profiles", "photometric_cost")
    alternating = alternate(parent) if parent else None  # before this process opens the GPU
    out = measure()
    if alternating:
        out["alternating"] = alternating
    if res:
        out["resources"] = [row for row in resources(res) if "icp_iterate" in row[0] or "raycast_kernel" in row[0]]
    with open(stem + ".json", "w") as f:
        json.dump(out, f, indent=1)
    write_md(stem + ".md", out)


if __name__ == "__main__":
    main()
