"""Cost of point-to-SDF tracking (profiles/point_sdf_cost.md, .json): per tracked frame at 640 x 480, the "sdf" tracker
(device_point_sdf.point_sdf_run) next to "icp" mode's ray-cast with normals plus ICP run (device_raycast.raycast,
device_icp.icp_run) from the same process, for 128^3 and 256^3 models.  The frames are those of
tools/photometric_cost.py (synthetic.depth_image fused at the identity, the second frame 2 px to the side and 8 mm
nearer, tracked from the identity).  Iterations (4, 4, 6) at strides (4, 2, 1): 15 launches and one copy back per run.
Device time between HIP events after a warm-up call, the two trackers alternating, best of REPS with the range of the
REPS.
  * one iteration by stride: (t21 - t1) / 20 of runs with 21 and with 1 iteration at that stride, both trackers
  * a tracked frame of SequenceFusion3d: its own tracking step on a model that holds frame 0, "sdf" and "icp"
  * with --resources FILE (hipcc -Rpass-analysis=kernel-resource-usage of csrc/lsf_point_sdf.hip and lsf_icp.hip,
    concatenated): the new instantiations beside the strided ICP kernels'
  * with --moved BEFORE AFTER (the same log of lsf_icp.hip and lsf_raycast.hip at the parent commit and now): whether
    the kernels of the two files whose shared code moved into headers kept their figures
  * the accuracy table of the restatement (tests/point_sdf_restatement.py on tests/moving_part_scene.py) is computed on
    the CPU in the same call
usage: point_sdf_cost.py [--resources FILE] [--moved BEFORE AFTER] [--render] [OUT_STEM]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from photometric_cost import load, offset  # noqa: E402
from pyramid_photometric_cost import resources  # noqa: E402

REPS, SIZES, STRIDES = 20, (128, 256), (4, 2, 1)


def accuracy():
    """the final pose errors of the restatement against a 48^3 model of the moving-part scene's undisturbed frame:
    {name: (translation m, rotation rad)}"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import fusion_restatement as F
    import fusion_scene as S
    import moving_part_scene as M
    import point_sdf_restatement as P
    import robust_icp_restatement as RR
    off = S.offset(48)
    t, w = F.empty_model((48,) * 3)
    t, w, _ = F.fuse_depth(t, w, M.render(np.zeros(6), moved=False), M.K, 1.0, off, np.zeros(6))
    rows = {}
    for moved in (True, False):
        for name, loss in (("least squares", None), ("huber", RR.Loss("huber", M.HUBER_SCALE)),
                           ("tukey", RR.Loss("tukey", M.TUKEY_SCALE))):
            twist = P.track(t, w, M.live(moved), M.K, 1.0, np.zeros(6), off, M.ITERATIONS, M.STRIDES, loss=loss)[1]
            rows[name + ("" if moved else ", nothing moved")] = M.pose_error(twist)
    return dict(changed_pixels=M.changed_pixels(), rows=rows)


def alternating(torch, fns, reps=REPS):
    """{name: device ms per repeat} of the calls in fns, one after the other within every repeat, after a warm-up"""
    for fn in fns.values():
        fn()
    out = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            out[name].append(a.elapsed_time(b))
    return out


def stat(ms):
    return dict(device_ms=min(ms), device_spread_ms=[min(ms), max(ms)])


def measure():
    np, torch, lsf, device_icp, device_raycast, synthetic, gen, cam = load(ROOT)
    from levelsetfusion_python_amd import device_point_sdf
    zero = np.zeros(6)
    first = synthetic.depth_image()
    live, code = gen.device_depth(synthetic.depth_image(shift_px=2.0, nearer_m=0.008))
    out = dict(rows={}, last_records={})
    for n in SIZES:
        off = offset(np, n)
        vol = lsf.fusion.CanonicalVolume(n)
        vol.integrate_depth(first, cam, zero, off)

        def cast():
            return device_raycast.raycast(vol.tsdf, vol.weight, cam, zero, off, normals=True)

        pd, pn, hits = cast()

        def sdf(iterations=(4, 4, 6), strides=STRIDES):
            return device_point_sdf.point_sdf_run(vol.tsdf, vol.weight, live, code, cam, off, zero,
                                                  iterations=iterations, strides=strides)

        def icp(iterations=(4, 4, 6), strides=STRIDES):
            return device_icp.icp_run(live, code, pd, pn, cam, zero, None, iterations, strides)

        def frame(mode):
            seq = lsf.SequenceFusion3d(cam, n, off, tracking_reference=mode)
            seq.integrate(first)
            if mode == "icp":
                return lambda: seq._track_icp(live, code, zero)
            return lambda: seq.sdf_tracker.track(live, code, seq.canonical.tsdf, seq.canonical.weight, off, zero)

        fns = {"sdf run": sdf, "icp run": icp, "raycast": cast, "raycast + icp run": lambda: (cast(), icp()),
               "frame sdf": frame("sdf"), "frame icp": frame("icp")}
        for s in STRIDES:
            for count in (1, 21):
                fns["sdf stride %d x%d" % (s, count)] = lambda s=s, c=count: sdf((c,), (s,))
                fns["icp stride %d x%d" % (s, count)] = lambda s=s, c=count: icp((c,), (s,))
        for name, ms in alternating(torch, fns).items():
            key = "%d %s" % (n, name)
            out["rows"][key] = stat(ms)
            print(key, json.dumps(out["rows"][key]), flush=True)
        for name, records in (("sdf", sdf()[1]), ("icp", icp()[1])):
            r = device_icp.unpack_record(records[-1])
            out["last_records"]["%d %s" % (n, name)] = dict(count=r["count"], no_sample=r["angle_rejected"],
                                                            skipped=r["skipped"], hits=int(hits.item()))
        del vol, pd, pn
    return out


def write_md(path, out):
    rows = out["rows"]

    def ms(key):
        return "%.3f ms (%.3f–%.3f)" % (rows[key]["device_ms"], *rows[key]["device_spread_ms"])

    def per(n, tracker, s):
        return (rows["%d %s stride %d x21" % (n, tracker, s)]["device_ms"] -
                rows["%d %s stride %d x1" % (n, tracker, s)]["device_ms"]) / 20.0

    lines = ["# Cost of point-to-SDF tracking (MI355X)", "",
             "`tools/point_sdf_cost.py` (raw numbers: `point_sdf_cost.json`), one GPU call.  The frames are those of",
             "`profiles/photometric_cost.md`: `synthetic.depth_image()` fused into the model at the identity, the second",
             "frame (2 px to the side, 8 mm nearer) tracked from the identity, 640 x 480, 4 mm voxels.  Iterations",
             "(4, 4, 6) at strides (4, 2, 1): 15 launches and one copy back per run.  Device time between HIP events",
             "around the call, after a warm-up call, the rows of a model alternating within every repeat, best of %d" % REPS,
             "with the range of the %d in brackets." % REPS, "",
             "| per tracked frame | 128³ | 256³ |", "|---|---|---|"]
    for label, key in (("\"sdf\": `point_sdf_run`", "sdf run"), ("\"icp\": ray-cast with normals", "raycast"),
                       ("\"icp\": `icp_run`", "icp run"), ("\"icp\": ray-cast + `icp_run`, one window", "raycast + icp run"),
                       ("`SequenceFusion3d(\"sdf\")`'s tracking step", "frame sdf"),
                       ("`SequenceFusion3d(\"icp\")`'s tracking step", "frame icp")):
        lines.append("| %s | %s |" % (label, " | ".join(ms("%d %s" % (n, key)) for n in SIZES)))
    lines += ["", "| one iteration, (t21 - t1) / 20 | " + " | ".join("%d³ sdf | %d³ icp" % (n, n) for n in SIZES) + " |",
              "|---|" + "---|" * (2 * len(SIZES))]
    for s in STRIDES:
        lines.append("| stride %d | " % s + " | ".join("%.4f ms | %.4f ms" % (per(n, "sdf", s), per(n, "icp", s))
                                                        for n in SIZES) + " |")
    lines.append("")
    for n in SIZES:
        ratio = rows["%d sdf run" % n]["device_ms"] / rows["%d raycast + icp run" % n]["device_ms"]
        q, i = out["last_records"]["%d sdf" % n], out["last_records"]["%d icp" % n]
        lines.append("- %d³: the \"sdf\" run takes %.2f of the ray-cast plus ICP run.  Last iteration: %d pairs (%d pixels "
                     "without a valid sample) against ICP's %d pairs from %d prediction hits."
                     % (n, ratio, q["count"], q["no_sample"], i["count"], i["hits"]))
    n = SIZES[-1]
    lines += ["", "A stride-4 launch has 80 tiles for its 256 workgroups, so its row is the fixed part of an iteration: the",
              "launch and the prologue, which combines the partials and solves and composes the 6 x 6 system on one",
              "thread.  Both trackers share it, and it is most of every iteration.  What the body adds at full",
              "resolution is the stride-1 row less the stride-4 row: %.1f us with 16 gathers a pixel against ICP's %.1f us"
              % (1e3 * (per(n, "sdf", 1) - per(n, "sdf", 4)), 1e3 * (per(n, "icp", 1) - per(n, "icp", 4))),
              "with 4, at %d³.  The run is therefore bound by its 15 launch-and-solve steps, not by the gathers, and it" % n,
              "costs %.3f ms more than ICP's run while the ray-cast it does without costs %.3f ms."
              % (rows["%d sdf run" % n]["device_ms"] - rows["%d icp run" % n]["device_ms"],
                 rows["%d raycast" % n]["device_ms"]), ""]
    if "resources" in out:
        lines += ["**Compiler resources** (`hipcc -O3 --offload-arch=gfx950 -ffp-contract=off "
                  "-Rpass-analysis=kernel-resource-usage`, 256 lanes per workgroup; the new instantiations of",
                  "`csrc/lsf_point_sdf.hip`, then the strided ICP kernels of `csrc/lsf_icp.hip`):", "",
                  "| kernel | VGPRs | AGPRs | SGPR spills | VGPR spills | scratch, bytes / lane | waves / SIMD |",
                  "|---|---|---|---|---|---|---|"]
        for row in out["resources"]:
            lines.append("| `%s` | %d | %d | %d | %d | %d | %d |" % tuple(row))
        lines += ["", "No instantiation spills a vector register to memory.  The scratch of every row is the prologue's 6 x 6",
                  "solve on one thread, which the strided ICP kernels and the finishing kernel have too: the new kernel",
                  "has none of its own.  Its body keeps the 8 corner values, their lerps and differences live beside the",
                  "30 float64 sums and the pose; the compiler fills the 256 VGPRs and parks 64 to 84 values in AGPRs",
                  "(register-to-register moves) and a few scalars in lanes of a vector register (SGPR spills, no memory",
                  "traffic either), at one wave per SIMD.  The launch asks for no more: at most 256 workgroups of four",
                  "waves on 256 compute units of four SIMDs.", ""]
    if "moved" in out:
        m = out["moved"]
        lines += ["**The moved code.**  `csrc/lsf_icp_shared.h` and `csrc/lsf_tsdf_sample.h` hold what `lsf_icp.hip` and",
                  "`lsf_raycast.hip` share with the new file, moved with its internal linkage.  Of the %d kernels of the" % m["kernels"],
                  "two files, %d keep the parent commit's VGPRs, AGPRs, spills, scratch and occupancy%s" %
                  (m["same"], "." if not m["changed"] else "; changed: " + ", ".join("`%s`" % k for k in m["changed"]) + "."),
                  ""]
    acc = out["accuracy"]
    lines += ["**Accuracy of the restatement on the CPU** (`tests/point_sdf_restatement.py`; the model is",
              "`tests/moving_part_scene.py`'s undisturbed frame fused into 48³ at the zero twist, the live frame at half a",
              "`fusion_scene.STEP` with `SPHERES[1]` moved by (8, 0, -8) mm, which changes %d of 19200 pixels;" % acc["changed_pixels"],
              "iterations (4, 4, 6) over strides (4, 2, 1), Huber at 1 mm, Tukey at 3 mm; the errors are the norms of the",
              "translation and of the rotation half of twist - truth):", "",
              "| loss | translation error | rotation error |", "|---|---|---|"]
    for name, (t, r) in acc["rows"].items():
        lines.append("| %s | %.3g m | %.3g rad |" % (name, t, r))
    lines += ["", "`tests/test_point_sdf_host.py` holds Tukey to twice its error here.", ""]
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    args, res, moved = sys.argv[1:], None, None
    while args[:1] in (["--resources"], ["--moved"]):
        if args[0] == "--resources":
            res, args = args[1], args[2:]
        else:
            moved, args = args[1:3], args[3:]
    render = args[:1] == ["--render"]  # the report again from OUT_STEM.json, without a device
    stem = args[-1] if args[render:] else os.path.join(ROOT, "profiles", "point_sdf_cost")
    if render:
        with open(stem + ".json") as f:
            return write_md(stem + ".md", json.load(f))
    out = measure()
    out["accuracy"] = accuracy()
    if res:
        table = resources(res)
        out["resources"] = [r for r in table if "point_sdf_iterate" in r[0]] + \
            [r for r in table if "icp_iterate" in r[0] and "<StridedSource" in r[0]]
    if moved:
        before, after = (sorted(resources(path)) for path in moved)
        changed = sorted({r[0] for r in before if r not in after} | {r[0] for r in after if r not in before})
        out["moved"] = dict(kernels=len(before), same=len([r for r in before if r in after]), changed=changed)
    with open(stem + ".json", "w") as f:
        json.dump(out, f, indent=1)
    write_md(stem + ".md", out)


if __name__ == "__main__":
    main()
