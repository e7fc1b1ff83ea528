"""Cost of the moving volume (profiles/moving_volume_cost.md, .json).
1. lsf_volume_shift (device_volume_shift.shift) at 128^3 and 256^3, with and without the colour volume, for the shifts
   (8, 0, 0), (3, 0, 0), (0, 8, 0), (0, 0, 8) and (5, -3, 2), next to torch.clone of the same tensors in the same run: a
   plain copy moves at least as many bytes, since the shift reads only what it retains.  The figures and the timing
   method are tools/colour_cost.py's (queued, single, host); every call alternates with the others within a repetition.
2. One streamed shift at 256^3 on the sphere scene of the tests (tests/fusion_scene.py): CanonicalVolume.shift with
   stream_mesh (up to three mesh extractions and their copies to the host) next to the same shift without, host clock
   around the call and a device wait.
3. A whole frame of SequenceFusion3d(tracking_reference="icp") at 256^3 on that scene with and without a moving_volume,
   host clock per integrate() with a device wait, the frames that shifted apart from those that stayed.
4. The pose errors of tests/test_gpu_volume_shift.py's sequence in the moving window and in the fixed volume, and the
   margin the test allows between them.
usage: moving_volume_cost.py [OUT_STEM]"""
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
import fusion_scene as S  # noqa: E402
import levelsetfusion_python_amd as lsf  # noqa: E402
from levelsetfusion_python_amd import device_volume_shift  # noqa: E402

SHIFTS = ((8, 0, 0), (3, 0, 0), (0, 8, 0), (0, 0, 8), (5, -3, 2))
PEAK = 8e12  # HBM3E, bytes per second
STREAM_SHIFT, STREAM_REPS = (80, -90, -110), 7  # each leaving slab reaches into what frame 0 observed
SEQUENCE_FRAMES, SEQUENCE_THRESHOLD, SEQUENCE_ANCHOR = 10, 3.0, (0.0, 0.0, 0.53)  # CC.offset centres z = 0.53 m


def name_of(s):
    return "shift(%d, %d, %d)" % s


def shift_bytes(n, s, colour):
    """bytes lsf_volume_shift reads (the retained voxels) and writes (every voxel)"""
    kept = int(np.prod([max(0, n - abs(v)) for v in s]))
    per = 24 if colour else 8
    return per * kept + per * n ** 3


def kernel_rows(blocker):
    out = []
    for n in (128, 256):
        for colour in (False, True):
            rng = torch.Generator(device="cuda").manual_seed(n)
            t, w, ot, ow = (torch.rand((n, n, n), device="cuda", generator=rng) for _ in range(4))
            c, oc = ((torch.rand((n, n, n, 4), device="cuda", generator=rng) for _ in range(2)) if colour
                     else (None, None))
            fns = {name_of(s): (lambda s=s: device_volume_shift.shift(t, w, c, ot, ow, oc, s)) for s in SHIFTS}
            fns["clone"] = (lambda: (t.clone(), w.clone(), c.clone())) if colour else (lambda: (t.clone(), w.clone()))
            m = CC.measure(fns, blocker)
            clone_bytes = 2 * (24 if colour else 8) * n ** 3
            row = dict(n=n, colour=colour, clone=m["clone"], clone_bytes=clone_bytes,
                       clone_fraction_of_peak=clone_bytes / (m["clone"]["queued"]["median"] * 1e-6) / PEAK, shifts=[])
            for s in SHIFTS:
                r = m[name_of(s)]
                b = shift_bytes(n, s, colour)
                row["shifts"].append(dict(shift=list(s), bytes=b, fraction_of_peak=b / (r["queued"]["median"] * 1e-6) / PEAK,
                                          ratio_to_clone=r["queued"]["median"] / m["clone"]["queued"]["median"], **r))
            out.append(row)
            print(json.dumps(row), flush=True)
            del fns, t, w, ot, ow, c, oc
            torch.cuda.empty_cache()
    return out


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def streamed_shift(n=256):
    """one shift of a 256^3 model that holds frame 0 of the sphere scene: streamed and not, host clock"""
    off = CC.offset(n)
    depth = S.frames(1)[0]
    raw = dict(streamed=[], plain=[])
    faces = chunks = 0
    for rep in range(STREAM_REPS + 1):  # the first repetition warms up (and allocates the spare buffers' pages)
        for kind in ("streamed", "plain"):
            vol = lsf.fusion.CanonicalVolume(n)
            vol.integrate_depth(depth, CC.CAM, S.true_twist(0), off)
            vol.shift((1, 0, 0), off)  # the spare buffers exist before the timed call
            ms, (_, got) = wall_ms(lambda: vol.shift(STREAM_SHIFT, off, stream_mesh=kind == "streamed"))
            if rep:
                raw[kind].append(ms)
            if kind == "streamed":
                faces, chunks = sum(len(c[1]) for c in got), len(got)
            del vol
    return dict(n=n, shift=list(STREAM_SHIFT), chunks=chunks, streamed_faces=faces,
                streamed_ms=CC.stats(raw["streamed"]), plain_ms=CC.stats(raw["plain"]))


def sequence_frames(n=256):
    """host clock per integrate() of the sphere scene's frames at n^3, "icp" tracking: without a moving volume, and with
    one (stayed / shifted frames apart)"""
    frames = S.frames(SEQUENCE_FRAMES)
    out = {}
    for kind in ("fixed", "moving"):
        policy = lsf.fusion.MovingVolume(SEQUENCE_THRESHOLD, SEQUENCE_ANCHOR) if kind == "moving" else None
        for attempt in range(2):  # the first pass warms up
            seq = lsf.SequenceFusion3d(CC.CAM, n, CC.offset(n), tracking_reference="icp", moving_volume=policy)
            times = [wall_ms(lambda d=d: seq.integrate(d))[0] for d in frames]
        records = seq.frame_records[1:]
        ms = np.array(times[1:])  # frame 0 is not tracked
        if kind == "fixed":
            out["fixed_ms"] = CC.stats(ms)
        else:
            moved = np.array([r["shift"] != (0, 0, 0) for r in records])
            out["moving_stayed_ms"] = CC.stats(ms[~moved])
            out["moving_shifted_ms"] = CC.stats(ms[moved])
            out["shifted_frames"] = int(moved.sum())
            out["streamed_faces_per_shift"] = float(np.mean([r["streamed_faces"] for r in records if r["shift"] != (0, 0, 0)]))
        del seq
        torch.cuda.empty_cache()
    return dict(n=n, frames=SEQUENCE_FRAMES, threshold_voxels=SEQUENCE_THRESHOLD, **out)


def pose_errors():
    """the test's sequence (tests/moving_volume_scene.py): largest pose error over the frames in the moving window and in
    the fixed volume that holds the whole path, and the test's margin"""
    import moving_volume_scene as MS
    import test_gpu_volume_shift as T
    policy = lsf.fusion.MovingVolume(MS.THRESHOLD, MS.ANCHOR)
    seq = lsf.SequenceFusion3d(T._camera(), MS.WINDOW, MS.WINDOW_OFFSET, voxel_size=MS.VOXEL,
                               narrow_band_width_voxels=MS.BAND, tracking_reference="icp", moving_volume=policy)
    for d in T._frames(MS.FRAMES)[0]:
        seq.integrate(d)
    (mt, mr), (ft, fr) = T._pose_errors(seq.twists), T._pose_errors(T._fixed_run(True).twists)
    return dict(frames=MS.FRAMES, shifts=sum(r["shift"] != (0, 0, 0) for r in seq.frame_records),
                moving_translation=float(mt.max()), moving_rotation=float(mr.max()),
                fixed_translation=float(ft.max()), fixed_rotation=float(fr.max()),
                largest_excess_translation=float((mt - ft).max()), largest_excess_rotation=float((mr - fr).max()),
                margin_translation=T.MARGIN_T, margin_rotation=T.MARGIN_R)


def write_md(path, kernel, streamed, sequence, pose):
    lines = ["# Cost of the moving volume (MI355X)", "",
             "`tools/moving_volume_cost.py` (raw numbers: `moving_volume_cost.json`).  The timing method and the three",
             "figures are `tools/colour_cost.py`'s: *queued* is device time per call with the host off the critical path",
             "(%d calls enqueued behind several ms of other device work, HIP events around them), *single* is HIP events" % CC.QUEUE,
             "around one call on an idle stream with the wrapper's checks inside the window, *host* is the host clock",
             "around the enqueue.  Medians of %d repetitions after %d warm-up calls; the calls of a table alternate within" %
             (CC.REPS, CC.WARMUP),
             "every repetition.", "",
             "## `lsf_volume_shift` next to `torch.clone` of the same tensors", "",
             "The shift reads the retained voxels and writes every voxel (8 B per voxel, 24 B with the colour volume); the",
             "clone reads and writes every voxel, so it moves at least as many bytes.  `of peak` is bytes moved over the",
             "queued time over 8 TB/s.  `clone spread` is the interquartile range of the clone's own queued figures: the",
             "run-to-run spread the shift is held against.", "",
             "| volume | colour | call | queued | single | host | bytes | of peak | queued / clone | clone spread |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for row in kernel:
        cl = row["clone"]
        spread = cl["queued"]["p75"] - cl["queued"]["p25"]
        lines.append("| %d³ | %s | clone | %.1f µs | %.1f µs | %.1f µs | %.1f MB | %.0f %% | 1.00 | %.2f µs |"
                     % (row["n"], "yes" if row["colour"] else "no", cl["queued"]["median"], cl["single"]["median"],
                        cl["host"]["median"], row["clone_bytes"] / 1e6, 100 * row["clone_fraction_of_peak"], spread))
        for r in row["shifts"]:
            lines.append("| %d³ | %s | shift (%d, %d, %d) | %.1f µs | %.1f µs | %.1f µs | %.1f MB | %.0f %% | %.2f | |"
                         % (row["n"], "yes" if row["colour"] else "no", *r["shift"], r["queued"]["median"],
                            r["single"]["median"], r["host"]["median"], r["bytes"] / 1e6, 100 * r["fraction_of_peak"],
                            r["ratio_to_clone"]))
    def span(row):
        ratios = [r["ratio_to_clone"] for r in row["shifts"]]
        return "%.2f to %.2f at %d³%s" % (min(ratios), max(ratios), row["n"], " with colour" if row["colour"] else "")

    lines += ["", "The aim was a shift that costs no more than the clone, within the clone's own spread.  Queued, the shift",
              "takes " + ", ".join(span(row) for row in kernel) + " of the clone's time (the clone is one launch per",
              "tensor, three with the colour volume; the shift is one).  Above the clone by more than its spread: " +
              (", ".join("%d³%s shift (%d, %d, %d) by %.1f µs" % (row["n"], " with colour" if row["colour"] else "", *r["shift"],
                                                                   r["queued"]["median"] - row["clone"]["queued"]["median"])
                         for row in kernel for r in row["shifts"]
                         if r["queued"]["median"] - row["clone"]["queued"]["median"] >
                         row["clone"]["queued"]["p75"] - row["clone"]["queued"]["p25"]) or "none") + ".",
              "A row is a wave's unit of work: at 128³ a row of tsdf or weight is 32 four-voxel groups, half a wave.",
              "", "Misaligned rows against aligned ones, queued: shift (3, 0, 0) over shift (8, 0, 0) is " +
              ", ".join("%.2f at %d³%s" % (row["shifts"][1]["queued"]["median"] / row["shifts"][0]["queued"]["median"],
                                           row["n"], " with colour" if row["colour"] else "") for row in kernel) + ".",
              "", "## One streamed shift at %d³" % streamed["n"], "",
              "A model that holds frame 0 of the sphere scene (`tests/fusion_scene.py`), shifted by (%d, %d, %d): host clock"
              % tuple(streamed["shift"]),
              "around `CanonicalVolume.shift` and a device wait, median of %d.  Streaming meshes the leaving boxes (%d"
              % (streamed["streamed_ms"]["count"], streamed["chunks"]),
              "chunks with a face, %d faces) with one host read of the totals each and copies them to the host."
              % streamed["streamed_faces"], "",
              "| | wall time |", "|---|---|",
              "| shift with `stream_mesh` | %.2f ms |" % streamed["streamed_ms"]["median"],
              "| shift alone | %.2f ms |" % streamed["plain_ms"]["median"], "",
              "## A whole frame at %d³" % sequence["n"], "",
              "`SequenceFusion3d(tracking_reference=\"icp\")` over %d frames of the sphere scene, host clock per" % sequence["frames"],
              "`integrate()` with a device wait, frames 1 and later; the moving volume has a threshold of %.0f voxels and"
              % sequence["threshold_voxels"],
              "streams (%d frames shifted, %.0f faces streamed per shift on average)."
              % (sequence["shifted_frames"], sequence["streamed_faces_per_shift"]), "",
              "| | median per frame |", "|---|---|",
              "| without `moving_volume` | %.2f ms |" % sequence["fixed_ms"]["median"],
              "| with, frames that stayed | %.2f ms |" % sequence["moving_stayed_ms"]["median"],
              "| with, frames that shifted | %.2f ms |" % sequence["moving_shifted_ms"]["median"], "",
              "## Pose error in the moving window", "",
              "`tests/test_gpu_volume_shift.py`, `test_a_sequence_in_a_moving_volume`: %d frames of" % pose["frames"],
              "`tests/moving_volume_scene.py`, %d shifts.  Norms of the translation and rotation parts of twist - truth," % pose["shifts"],
              "largest over the frames; the excess is the largest per-frame difference moving - fixed.", "",
              "| | translation | rotation |", "|---|---|---|",
              "| moving window (48³) | %.6f m | %.6f rad |" % (pose["moving_translation"], pose["moving_rotation"]),
              "| fixed volume holding the whole path | %.6f m | %.6f rad |" % (pose["fixed_translation"], pose["fixed_rotation"]),
              "| largest excess per frame | %.6f m | %.6f rad |" % (pose["largest_excess_translation"], pose["largest_excess_rotation"]),
              "| margin the test allows | %.6f m | %.6f rad |" % (pose["margin_translation"], pose["margin_rotation"]),
              "", ""]
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    stem = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "moving_volume_cost")
    os.makedirs(os.path.dirname(os.path.abspath(stem)), exist_ok=True)
    blocker = torch.zeros(CC.BLOCKER_FLOATS, dtype=torch.float32, device="cuda")
    kernel = kernel_rows(blocker)
    del blocker
    torch.cuda.empty_cache()
    streamed = streamed_shift()
    print(json.dumps(streamed), flush=True)
    sequence = sequence_frames()
    print(json.dumps(sequence), flush=True)
    pose = pose_errors()
    print(json.dumps(pose), flush=True)
    with open(stem + ".json", "w") as f:
        json.dump(dict(kernel=kernel, streamed_shift=streamed, sequence=sequence, pose=pose, warmup=CC.WARMUP,
                       reps=CC.REPS, queue=CC.QUEUE), f, indent=1)
    write_md(stem + ".md", kernel, streamed, sequence, pose)


if __name__ == "__main__":
    main()
