"""Cost of point-to-SDF tracking with the colour term and on the depth pyramid (profiles/point_sdf_colour_cost.md,
.json): per tracked frame at 640 x 480 against 128^3 and 256^3 models with colour, the plain run
(device_point_sdf.point_sdf_run), the strided joint run (point_sdf_run_photometric), the pyramid run and the pyramid
joint run (point_sdf_run_pyramid, with the builds of the depth pyramid and of the intensity pyramid they need), and a
tracked frame of each in a SequenceFusion3d.  The frames are those of tools/photometric_cost.py: synthetic.depth_image
and a colour image painted by pixel position fused at the identity (colour_band 0.25), the second frame 2 px to the
side and 8 mm nearer, tracked from the identity.  Iterations (4, 4, 6), strides (4, 2, 1) or the default DepthPyramid:
15 launches and one copy back per run.  Device time between HIP events after a warm-up call, the rows of a model
alternating within every repeat, best of REPS with the range of the REPS.
  * with --resources FILE (hipcc -Rpass-analysis=kernel-resource-usage of csrc/lsf_point_sdf.hip): every instantiation's
    registers, spills, scratch and occupancy
  * with --noisy: tests/noisy_scene.py, five frames at 48^3, through the restated strided and pyramid trackers
    (tests/point_sdf_restatement.py, tests/point_sdf_colour_restatement.py), on the CPU
usage: point_sdf_colour_cost.py [--resources FILE] [--noisy] [--render] [OUT_STEM]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from photometric_cost import colour_image, load, offset  # noqa: E402
from point_sdf_cost import alternating, stat  # noqa: E402
from pyramid_photometric_cost import resources  # noqa: E402

SIZES, LAMBDA, COLOUR_BAND = (128, 256), 0.1, 0.25
ROWS = (("plain: `point_sdf_run`", "plain"), ("strided joint: `point_sdf_run_photometric`", "strided joint"),
        ("depth pyramid build", "depth pyramid"), ("intensity pyramid build", "intensity pyramid"),
        ("pyramid: `point_sdf_run_pyramid`", "pyramid"), ("pyramid joint: `point_sdf_run_pyramid`", "pyramid joint"),
        ("pyramid joint with both builds", "pyramid joint + builds"),
        ("`SequenceFusion3d(\"sdf\")`'s tracking step, plain", "frame plain"),
        ("the same, strided joint tracker", "frame strided joint"), ("the same, pyramid tracker", "frame pyramid"),
        ("the same, pyramid joint tracker", "frame pyramid joint"))


def noisy():
    """the worst pose errors over frames 1 .. 4 of tests/noisy_scene.py at 48^3 through the restated "sdf" sequence,
    strided and on the default DepthPyramid: {name: (translation m, rotation rad)}"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import depth_pyramid_restatement as DP
    import fusion_restatement as F
    import fusion_scene as S
    import noisy_scene as NS
    import point_sdf_colour_restatement as PC
    import point_sdf_restatement as P
    n, count = 48, 5
    frames, off = NS.frames(count), S.offset(48)
    rows = {}
    for name in ("strided", "pyramid"):
        t, w = F.empty_model((n,) * 3)
        twist, worst = np.zeros(6), np.zeros(2)
        for k, depth in enumerate(frames):
            if k and name == "strided":
                twist = P.track(t, w, depth, S.K, NS.RATIO, twist, off)[1]
            elif k:
                depths, _, intr = DP.pyramid(depth, NS.RATIO, S.K)
                twist = PC.track_pyramid(t, w, depths, intr, twist, off)[1]
            err = np.abs(twist - S.true_twist(k))
            worst = np.maximum(worst, [err[:3].max(), err[3:].max()])
            t, w, _ = F.fuse_depth(t, w, depth, S.K, NS.RATIO, off, twist)
        rows[name] = [float(worst[0]), float(worst[1])]
    return rows


def measure():
    np, torch, lsf, device_icp, _, synthetic, gen, cam = load(ROOT)
    from levelsetfusion_python_amd import device_point_sdf
    from levelsetfusion_python_amd.rigid_opt import DepthPyramid, IntensityPyramid, PointToSdf3d
    zero = np.zeros(6)
    first, first_colour = synthetic.depth_image(), colour_image(np)
    second = synthetic.depth_image(shift_px=2.0, nearer_m=0.008)
    live, code = gen.device_depth(second)
    image = torch.from_numpy(colour_image(np, 2.0)).cuda()
    dp, ip = DepthPyramid(), IntensityPyramid()
    out = dict(rows={}, last_records={})
    for n in SIZES:
        off = offset(np, n)
        vol = lsf.fusion.CanonicalVolume(n, colour=True)
        vol.integrate_depth(first, cam, zero, off, colour_image=first_colour, colour_band=COLOUR_BAND)
        levels, intensity = dp.build_device(live, code, cam), ip.build_device(image)

        def plain():
            return device_point_sdf.point_sdf_run(vol.tsdf, vol.weight, live, code, cam, off, zero)

        def strided_joint():
            return device_point_sdf.point_sdf_run_photometric(vol.tsdf, vol.weight, live, code, cam, off, zero,
                                                              colour=vol.colour, live_colour=image,
                                                              photometric_weight=LAMBDA)

        def pyramid(joint, build=False):
            lv = dp.build_device(live, code, cam) if build else levels
            it = (ip.build_device(image) if build else intensity) if joint else None
            kw = dict(colour=vol.colour, pyramid_intensity=it.buffer, photometric_weight=LAMBDA) if joint else {}
            return device_point_sdf.point_sdf_run_pyramid(vol.tsdf, vol.weight, lv.buffers[0], dp.levels, (480, 640),
                                                          cam, off, zero, **kw)

        def frame(**kw):
            tracker = PointToSdf3d(cam, **kw)
            seq = lsf.SequenceFusion3d(cam, n, off, tracking_reference="sdf", sdf_tracker=tracker, colour=True,
                                       colour_band=COLOUR_BAND)
            seq.integrate(first, first_colour)
            model = seq.canonical
            joint = dict(colour=model.colour, colour_image=image) if tracker.photometric_weight is not None else {}
            return lambda: tracker.track(live, code, model.tsdf, model.weight, off, zero, **joint)

        fns = {"plain": plain, "strided joint": strided_joint,
               "depth pyramid": lambda: dp.build_device(live, code, cam),
               "intensity pyramid": lambda: ip.build_device(image), "pyramid": lambda: pyramid(False),
               "pyramid joint": lambda: pyramid(True), "pyramid joint + builds": lambda: pyramid(True, True),
               "frame plain": frame(), "frame strided joint": frame(photometric_weight=LAMBDA),
               "frame pyramid": frame(pyramid=dp),
               "frame pyramid joint": frame(pyramid=dp, intensity_pyramid=ip, photometric_weight=LAMBDA)}
        for name, ms in alternating(torch, fns).items():
            key = "%d %s" % (n, name)
            out["rows"][key] = stat(ms)
            print(key, json.dumps(out["rows"][key]), flush=True)
        for name, records in (("plain", plain()[1]), ("strided joint", strided_joint()[1]),
                              ("pyramid", pyramid(False)[1]), ("pyramid joint", pyramid(True)[1])):
            r = device_icp.unpack_record(records[-1])
            out["last_records"]["%d %s" % (n, name)] = dict(count=r["count"], photometric_count=r["photometric_count"],
                                                            no_sample=r["angle_rejected"], skipped=r["skipped"])
        del vol
    return out


def write_md(path, out):
    rows = out["rows"]

    def ms(key):
        return "%.3f ms (%.3f–%.3f)" % (rows[key]["device_ms"], *rows[key]["device_spread_ms"])

    lines = ["# Cost of point-to-SDF tracking with a colour term and on the depth pyramid (MI355X)", "",
             "`tools/point_sdf_colour_cost.py` (raw numbers: `point_sdf_colour_cost.json`), one GPU call.  The frames are",
             "those of `profiles/photometric_cost.md` and `profiles/point_sdf_cost.md`: `synthetic.depth_image()` and a",
             "colour image painted by pixel position fused into a model with colour at the identity (`colour_band`",
             "%.2f), the second frame (2 px to the side, 8 mm nearer) tracked from the identity, 640 x 480, 4 mm" % COLOUR_BAND,
             "voxels, lambda %.1f.  Iterations (4, 4, 6) at strides (4, 2, 1) or on the default three-level" % LAMBDA,
             "`DepthPyramid`: 15 launches and one copy back per run.  Device time between HIP events around the call,",
             "after a warm-up call, the rows of a model alternating within every repeat, best of 20 with the range of",
             "the 20 in brackets.  No time here is a pass condition; `profiles/point_sdf_cost.md` and",
             "`profiles/pyramid_photometric_cost.md` hold the \"icp\" tracker's figures for the same frame size.", "",
             "| per tracked frame | " + " | ".join("%d³" % n for n in SIZES) + " |", "|---|" + "---|" * len(SIZES)]
    for label, key in ROWS:
        lines.append("| %s | %s |" % (label, " | ".join(ms("%d %s" % (n, key)) for n in SIZES)))
    lines.append("")
    for n in SIZES:
        last = out["last_records"]
        lines.append("- %d³, last iteration: " % n + "; ".join(
            "%s %d pairs, %d with a colour term, %d pixels without a valid sample" % (
                name, last["%d %s" % (n, name)]["count"], last["%d %s" % (n, name)]["photometric_count"],
                last["%d %s" % (n, name)]["no_sample"]) for name in ("plain", "strided joint", "pyramid",
                                                                      "pyramid joint")) + ".")
    if out.get("resources"):
        lines += ["", "**Compiler resources** (`hipcc -O3 --offload-arch=gfx950 -ffp-contract=off "
                  "-Rpass-analysis=kernel-resource-usage`, 256 lanes per workgroup; every kernel of "
                  "`csrc/lsf_point_sdf.hip`: the six of `lsf_point_sdf_run`, untouched, then the new ones):", "",
                  "| kernel | VGPRs | AGPRs | SGPR spills | VGPR spills | scratch, bytes / lane | waves / SIMD |",
                  "|---|---|---|---|---|---|---|"]
        for row in out["resources"]:
            lines.append("| `%s` | " % row[0] + " | ".join(str(v) for v in row[1:]) + " |")
        lines += ["",
                  "No instantiation spills to scratch memory.  The 304 bytes of every row are the prologue's 6 x 6 solve",
                  "on one thread, which the finishing kernels (`icp_finish_kernel`, no per-pixel body at all) have too.",
                  "The three strided joint kernels with a loss report 4 VGPR spills at the same 304 bytes: their",
                  "assembly holds those four values in AGPRs (`v_accvgpr_write_b32` / `v_accvgpr_read_b32`, marked",
                  "\"Reload Reuse\"), and it has the 169 scratch loads and stores of the finishing kernel, which every",
                  "kernel of the file has, and none beyond them.  SGPR spills go to lanes of",
                  "a vector register, no memory traffic either.  The geometric rows are finished before the colour",
                  "term is formed, so its 8 records, 8 luminances and second 6-vector reuse the registers of the SDF",
                  "sample and of J; every kernel stays at one wave per SIMD, which is all a launch of at most 256",
                  "workgroups of four waves asks of 256 compute units.  The six kernels of `lsf_point_sdf_run` keep",
                  "the figures of `profiles/point_sdf_cost.md`, and the 28 kernels of `csrc/lsf_icp.hip`, out of which",
                  "`PyramidSource` moved unchanged into `csrc/lsf_icp_shared.h`, report what they reported at the parent",
                  "commit in every column (the same log of that file before and after, compared line by line)."]
    if out.get("noisy"):
        lines += ["", "**Filtered depth on noisy frames** (CPU, the restatements: `tests/noisy_scene.py`, five frames at",
                  "48³, iterations (4, 4, 6), the worst error over frames 1 to 4; the pyramid is the default",
                  "`DepthPyramid`, bilateral radius 3).  Recorded, not asserted:", "",
                  "| \"sdf\" tracker | worst translation error | worst rotation error |", "|---|---|---|"]
        for name, label in (("strided", "strided, raw depth"), ("pyramid", "pyramid, filtered depth")):
            lines.append("| %s | %.3f mm | %.3g rad |" % (label, 1e3 * out["noisy"][name][0], out["noisy"][name][1]))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main(argv):
    args = list(argv)
    log = args.pop(args.index("--resources") + 1) if "--resources" in args else None
    flags = {a for a in args if a.startswith("--")}
    stem = ([a for a in args if not a.startswith("--")] or [os.path.join(ROOT, "profiles", "point_sdf_colour_cost")])[0]
    if "--render" in flags:
        with open(stem + ".json") as f:
            out = json.load(f)
    else:
        out = measure()
    if log:
        out["resources"] = [r for r in resources(log) if r[0].startswith("point_sdf_iterate_kernel")]
    if "--noisy" in flags:
        out["noisy"] = noisy()
    with open(stem + ".json", "w") as f:
        json.dump(out, f, indent=1)
    write_md(stem + ".md", out)


if __name__ == "__main__":
    main(sys.argv[1:])
