"""Cost of warped depth fusion (profiles/warped_fusion_cost.md, .json): device_fusion.integrate_depth_warped next to
device_fusion.integrate_depth_weighted and device_fusion.integrate_depth_colour -- whose kernels this entry point left as
they were -- in the same build and the same run, with the same arguments, at 128^3 and 256^3, on the painted sphere scene
of the tests (tests/colour_scene.py; 640 x 480, 4 mm voxels, 20-voxel band) and a model that already holds frame 0.  The
figures (queued, single, host) and the way they are taken are tools/colour_cost.py's; the four calls alternate within
every repetition.  The warp is a zero field (the warped call then computes what the call beside it computes) and a
smooth field of up to two voxels.
A second table times one whole non-rigid frame of SequenceFusion3d(nonrigid_optimizer=HierarchicalOptimizer3d(...)), host
clock from integrate() to its return (it ends with the record read, so the device is idle then), next to the same frame
without an optimizer, and the frame's three device stages on their own: the live volume, optimize() and the warped call.
usage: warped_fusion_cost.py [OUT_STEM [SUITE_RESULT]]    SUITE_RESULT: the test suite's closing line on the same
build, recorded at the end of the document"""
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

import colour_scene as CS  # noqa: E402
import deforming_scene as D  # noqa: E402
import fusion_scene as S  # noqa: E402
import levelsetfusion_python_amd as lsf  # noqa: E402
from colour_cost import CAM, QUEUE, REPS, WARMUP, BLOCKER_FLOATS, measure, offset  # noqa: E402
from levelsetfusion_python_amd import device_fusion, device_rigid  # noqa: E402
from levelsetfusion_python_amd.tsdf import generation as gen  # noqa: E402

NAMES = ("weighted", "warped", "colour", "warped_colour")
FRAME_REPS = 7
BAND = 0.25  # colour_band


def smooth_warp(n, amplitude=2.0):
    """a float32 (n, n, n, 3) field of slow sines, at most `amplitude` voxels per component"""
    g = torch.arange(n, dtype=torch.float32, device="cuda") * (2 * np.pi / n)
    z, y, x = torch.meshgrid(g, g, g, indexing="ij")
    return (amplitude * torch.stack([torch.sin(y + 0.3) * torch.cos(z), torch.sin(z + 1.1) * torch.cos(x),
                                     torch.sin(x + 2.0) * torch.cos(y)], dim=-1)).contiguous()


def calls(n, warp):
    """the four calls at n^3 on a model that holds frame 0 (carving on), and the warped colour call's record"""
    (d0, i0, _), (d1, i1, _) = CS.frames()[:2]
    off = offset(n)
    depth, code = gen.device_depth(d1)
    image = torch.from_numpy(i1.copy()).cuda()
    vol = lsf.fusion.CanonicalVolume(n, colour=True)
    vol.integrate_depth(d0, CAM, S.true_twist(0), off, colour_image=i0, carve=True, colour_band=BAND)
    t, w, c = vol.tsdf.clone(), vol.weight.clone(), vol.colour.clone()
    args = (depth, code, CAM, off, S.true_twist(1))
    fns = dict(
        weighted=lambda: device_fusion.integrate_depth_weighted(t, w, *args, carve=True),
        warped=lambda: device_fusion.integrate_depth_warped(t, w, *args, warp, carve=True),
        colour=lambda: device_fusion.integrate_depth_colour(t, w, c, *args, image, colour_band=BAND, carve=True),
        warped_colour=lambda: device_fusion.integrate_depth_warped(t, w, *args, warp, carve=True, colour=c,
                                                                   colour_image=image, colour_band=BAND))
    return fns, lambda: device_fusion.unpack_warped_record(fns["warped_colour"]().cpu().numpy())


def call_rows():
    out = []
    blocker = torch.zeros(BLOCKER_FLOATS, dtype=torch.float32, device="cuda")
    for n in (128, 256):
        for kind in ("zero", "smooth"):
            warp = torch.zeros((n, n, n, 3), dtype=torch.float32, device="cuda") if kind == "zero" else smooth_warp(n)
            fns, record = calls(n, warp)
            m = measure(fns, blocker)
            rec = record()
            row = dict(n=n, warp=kind, updated_fraction=(rec["fused"] + rec["carved"]) / n ** 3,
                       coloured_fraction=rec["coloured"] / n ** 3, warp_bytes=12 * n ** 3, **m)
            out.append(row)
            print(json.dumps(row), flush=True)
            del fns, record, warp
        torch.cuda.empty_cache()
    return out


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def frame_row(name, camera, n, off, frames, twist, band, voxel=0.004, images=None):
    """one whole frame 1 (frame 0 fused before the clock starts), FRAME_REPS fresh sequences of each kind"""
    colour = images is not None
    raw = dict(rigid=[], nonrigid=[], live=[], optimize=[], fuse=[])
    iterations = None
    for rep in range(FRAME_REPS + 1):  # the first builds the optimizer's plans and graphs and is not counted
        for kind in ("rigid", "nonrigid"):
            opt = lsf.HierarchicalOptimizer3d(**D.OPTIMIZER) if kind == "nonrigid" else None
            seq = lsf.SequenceFusion3d(camera, n, off, voxel_size=voxel, narrow_band_width_voxels=band,
                                       rigid_iterations=0, nonrigid_optimizer=opt, initial_twist=twist, carve=True,
                                       colour=colour)
            seq.integrate(frames[0], *((images[0],) if colour else ()))
            if kind == "nonrigid":  # the stages on their own, on the model as frame 1 meets it; the sequence's own
                model = seq.canonical  # optimizer, so the counted frame below meets it warmed as a running sequence's is
                depth, code = gen.device_depth(frames[1])
                ms_live, live = wall_ms(lambda: device_rigid.live_volume_3d(
                    depth, code, camera, seq.field_shape, seq.array_offset, twist, voxel_size=voxel,
                    narrow_band_width_voxels=band))
                ms_opt, psi = wall_ms(lambda: opt.optimize(model.tsdf, live))
                t, w = model.tsdf.clone(), model.weight.clone()
                c = model.colour.clone() if colour else None
                image = torch.from_numpy(np.ascontiguousarray(images[1])).cuda() if colour else None
                ms_fuse, _ = wall_ms(lambda: device_fusion.integrate_depth_warped(
                    t, w, depth, code, camera, seq.array_offset, twist, psi, voxel, band, carve=True, colour=c,
                    colour_image=image))
                iterations = opt.get_per_level_iteration_counts()
            ms, _ = wall_ms(lambda: seq.integrate(frames[1], *((images[1],) if colour else ())))
            if rep > 0:
                raw[kind].append(ms)
                if kind == "nonrigid":
                    raw["live"].append(ms_live), raw["optimize"].append(ms_opt), raw["fuse"].append(ms_fuse)
    row = dict(scene=name, n=n, colour=colour, iterations=iterations,
               **{k: float(np.median(v)) for k, v in raw.items()})
    print(json.dumps(row), flush=True)
    return row


def frame_rows():
    cam1 = gen.DepthCamera(intrinsics=gen.DepthCamera.Intrinsics(intrinsic_matrix=D.K), depth_unit_ratio=1.0)
    out = [frame_row("growing sphere (tests/deforming_scene.py)", cam1, D.N, D.OFFSET, D.frames(), D.TWIST, D.BAND,
                     D.VOXEL)]
    painted = CS.frames()[:2]
    depths, images = [f[0] for f in painted], [f[1] for f in painted]
    for n in (128, 256):  # both frames under frame 0's twist: the non-rigid step takes up the camera's motion
        out.append(frame_row("painted spheres (tests/colour_scene.py), colour", CAM, n, offset(n), depths,
                             S.true_twist(0), 20, images=images))
    return out


def write_md(path, table, frames, suite=None):
    def med(r, name, kind):
        return r[name][kind]["median"]

    def spread(kind):
        return max(r[k][kind]["p75"] - r[k][kind]["p25"] for r in table for k in NAMES)

    lines = ["# Cost of warped depth fusion (MI355X)", "",
             "`tools/warped_fusion_cost.py` (raw numbers: `warped_fusion_cost.json`).  Frame 1 of the painted sphere scene",
             "(`tests/colour_scene.py`) fused at its true twist, with carving, into a model that holds frame 0; 4 mm voxels,",
             "20-voxel band, `colour_band` %.2f.  `lsf_fusion_integrate_depth_warped` runs next to" % BAND,
             "`lsf_fusion_integrate_depth_weighted` and `lsf_fusion_integrate_depth_colour`, whose kernels it left unchanged,",
             "in the same build and the same run with the same arguments; the four calls alternate within each of the %d" % REPS,
             "repetitions after %d warm-up calls, and every figure is a median.  The widest interquartile range is %.1f µs" %
             (WARMUP, spread("queued")),
             "among the queued figures, %.1f µs among the single-call ones and %.1f µs among the host ones." %
             (spread("single"), spread("host")), "",
             "- *queued* is device time per call with the host off the critical path: %d calls enqueued behind several ms" % QUEUE,
             "  of other device work, HIP events around them, counted only when the host had finished enqueueing before the",
             "  device reached the first event.  It covers the fuse launch, the finishing launch and the gaps between them.",
             "- *single* is HIP events around one call on an idle stream: the Python wrapper's checks run inside the window.",
             "- *host* is the host clock around enqueueing one call, with no device wait: the wrapper alone.", "",
             "The warped call reads 12 B per voxel more than the call beside it: the voxel's three warp floats, whatever",
             "the voxel sees (`warp bytes`; the weighted call reads 8 B per voxel of model, and writes 8 B where a step",
             "updates).  The *zero* field makes it compute exactly what the call beside it computes; the *smooth* field",
             "moves every voxel's point by up to two voxels per axis.", "",
             "| volume | warp | queued: weighted | warped | ratio | colour | warped + colour | ratio | single: weighted | warped "
             "| colour | warped + colour | host: weighted | warped | colour | warped + colour | updated voxels "
             "| coloured voxels | warp bytes |",
             "|" + "---|" * 19]
    for r in table:
        lines.append("| %d³ | %s | %.1f µs | %.1f µs | %.2f | %.1f µs | %.1f µs | %.2f | %.1f µs | %.1f µs | %.1f µs | %.1f µs "
                     "| %.1f µs | %.1f µs | %.1f µs | %.1f µs | %.1f %% | %.2f %% | %.1f MB |"
                     % (r["n"], r["warp"], med(r, "weighted", "queued"), med(r, "warped", "queued"),
                        med(r, "warped", "queued") / med(r, "weighted", "queued"), med(r, "colour", "queued"),
                        med(r, "warped_colour", "queued"), med(r, "warped_colour", "queued") / med(r, "colour", "queued"),
                        med(r, "weighted", "single"), med(r, "warped", "single"), med(r, "colour", "single"),
                        med(r, "warped_colour", "single"), med(r, "weighted", "host"), med(r, "warped", "host"),
                        med(r, "colour", "host"), med(r, "warped_colour", "host"), 100 * r["updated_fraction"],
                        100 * r["coloured_fraction"], r["warp_bytes"] / 1e6))
    lines += ["", "## One whole non-rigid frame", "",
              "`SequenceFusion3d(nonrigid_optimizer=HierarchicalOptimizer3d(...), carve=True, rigid_iterations=0)` with the",
              "optimizer settings of `tests/deforming_scene.py` (`tikhonov_strength` 0.05, rate 0.3, at most 100 iterations a",
              "level, threshold 0.001, no gradient kernel): host clock around `integrate(frame 1)`, which ends with the record",
              "read, next to the same frame of a sequence without an optimizer; medians of %d fresh sequences after one" % FRAME_REPS,
              "uncounted round.  *live*, *optimize* and *fuse* are the frame's three stages run on their own on the same",
              "model, each with a device wait after it: `device_rigid.live_volume_3d`, `optimizer.optimize(model, live)` and",
              "`integrate_depth_warped`.  The staged optimize() is that optimizer's first call and pays its one-time set-up",
              "(plans, captured graphs); the frame's is its second, so a frame can take less than the stage.  *iterations* are",
              "optimize()'s per level, coarsest first.", "",
              "| scene | volume | frame without optimizer | frame with optimizer | live | optimize | fuse | iterations |",
              "|---|---|---|---|---|---|---|---|"]
    for r in frames:
        lines.append("| %s | %d³ | %.2f ms | %.2f ms | %.2f ms | %.2f ms | %.2f ms | %s |"
                     % (r["scene"], r["n"], r["rigid"], r["nonrigid"], r["live"], r["optimize"], r["fuse"],
                        ", ".join(str(i) for i in r["iterations"])))
    if suite:
        lines += ["", "## Test suite", "", "`python -m pytest tests` on an MI355X with this code: %s." % suite]
    lines += ["", ""]
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    table = call_rows()
    frames = frame_rows()
    stem = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "warped_fusion_cost")
    os.makedirs(os.path.dirname(os.path.abspath(stem)), exist_ok=True)
    with open(stem + ".json", "w") as f:
        json.dump(dict(rows=table, frames=frames, warmup=WARMUP, reps=REPS, queue=QUEUE, frame_reps=FRAME_REPS), f,
                  indent=1)
    write_md(stem + ".md", table, frames, sys.argv[2] if len(sys.argv) > 2 else None)


if __name__ == "__main__":
    main()
