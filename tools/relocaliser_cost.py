"""Cost of tracking quality and relocalisation (profiles/relocaliser_cost.md, .json).
1. device_relocaliser.encode at 160 x 120 and 640 x 480, with and without colour, into the default 30 x 40 coarse image
   (15 x 20 at 160 x 120): fusion_scene's depth rendered at the size, random bytes as colour.
2. device_relocaliser.query of that coarse image against a database of 16, 1024 and 4096 keyframes of 500 ferns of 4
   decisions (random codes), without harvest, and the bandwidth n * F bytes per queued call implies.
   The figures and the timing method are tools/colour_cost.py's (queued, single, host), the calls alternating within every
   repetition.
3. A tracked and fused frame of SequenceFusion3d at 128^3 ("icp" tracking, 640 x 480, fusion_scene) with
   relocaliser=Relocaliser() and without the keywords: host clock around integrate() and a device wait, the two sequences
   alternating within every repetition.  The run without is the code that did not change.
usage: relocaliser_cost.py [OUT_STEM]"""
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
import relocaliser_restatement as R  # noqa: E402
import levelsetfusion_python_amd as lsf  # noqa: E402
from levelsetfusion_python_amd import device_relocaliser as D  # noqa: E402

N = 128
FRAMES = 6
FRAME_REPS = 7
FERNS, DECISIONS = 500, 4
DEPTH_RANGE = (0.2, 4.0)
SIZES = (dict(name="160 x 120", shape=(120, 160), coarse=(15, 20)), dict(name="640 x 480", shape=(480, 640), coarse=(30, 40)))
DATABASES = (16, 1024, 4096)


def scene_depth(shape):
    h, w = shape
    K = np.array(S.K, dtype=np.float64)
    K[:2] *= w / 640.0
    return S.render(S.true_twist(0), w, h, K)


def encodes(blocker):
    rows = []
    for size in SIZES:
        h, w = size["shape"]
        depth = torch.from_numpy(scene_depth(size["shape"])).cuda()
        image = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda()
        plain = D.encode(depth, size["coarse"], DEPTH_RANGE)
        both = D.encode(depth, size["coarse"], DEPTH_RANGE, colour=image)
        fns = {"depth": lambda: D.encode(depth, size["coarse"], DEPTH_RANGE, 1.0, None, *plain),
               "depth and colour": lambda: D.encode(depth, size["coarse"], DEPTH_RANGE, 1.0, image, *both)}
        kernels = CC.measure(fns, blocker)
        record = D.unpack_encode_record(plain[2].cpu().numpy())
        rows.append(dict(name=size["name"], coarse="%d x %d" % size["coarse"], pixels=h * w, record=record,
                         bytes={"depth": h * w * 4, "depth and colour": h * w * 7}, kernels=kernels))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def queries(blocker):
    size = SIZES[1]
    coarse = D.encode(torch.from_numpy(scene_depth(size["shape"])).cuda(), size["coarse"], DEPTH_RANGE)[0]
    table = [torch.from_numpy(a).cuda() for a in R.fern_table(FERNS, DECISIONS, size["coarse"], DEPTH_RANGE, False, 0)]
    rng = np.random.default_rng(5)
    rows = []
    for n in DATABASES:
        codes = torch.from_numpy(rng.integers(0, 1 << DECISIONS, (n, FERNS), dtype=np.uint8)).cuda()
        size_n = torch.tensor([n], dtype=torch.int32, device="cuda")
        out = D.query(coarse, *table, codes, size_n)
        call = CC.measure({"query": lambda: D.query(coarse, *table, codes, size_n, 1, False, 1, *out)}, blocker)["query"]
        rows.append(dict(keyframes=n, ferns=FERNS, database_bytes=n * FERNS, call=call,
                         gb_per_s=n * FERNS / (call["queued"]["median"] * 1e-6) / 1e9))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def frames():
    """wall ms of integrate() per tracked and fused frame (k >= 1), with relocaliser= and without the keywords"""
    depth = [torch.from_numpy(S.render(S.true_twist(k))).cuda() for k in range(FRAMES)]
    settings = dict(tracking_reference="icp")
    times = {"without the keywords": [], "with relocaliser": []}
    states = []
    for rep in range(2 + FRAME_REPS):
        order = list(times) if rep % 2 == 0 else list(times)[::-1]
        for name in order:
            extra = dict(relocaliser=lsf.fusion.Relocaliser()) if name == "with relocaliser" else {}
            seq = lsf.fusion.SequenceFusion3d(CC.CAM, N, CC.offset(N), **settings, **extra)
            for k, d in enumerate(depth):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rec = seq.integrate(d)
                torch.cuda.synchronize()
                if rep >= 2 and k >= 1:
                    times[name].append((time.perf_counter() - t0) * 1e3)
                if extra:
                    states.append(rec["tracking_state"])
            del seq
    assert set(states) == {"tracking"}, set(states)  # the comparison is of frames that were tracked and fused
    return dict(n=N, frames_per_sequence=FRAMES, reps=FRAME_REPS, wall_ms={k: CC.stats(v) for k, v in times.items()})


def write_md(path, enc, qry, frame):
    lines = ["# Cost of tracking quality and relocalisation (MI355X)", "",
             "`tools/relocaliser_cost.py` (raw numbers: `relocaliser_cost.json`).  Nothing here had been measured before, so no",
             "target was set in advance; the numbers are reported.", "",
             "## `lsf_reloc_encode`", "",
             "float32 depth in metres (tests/fusion_scene.py rendered at the size), `depth_range = (0.2, 4.0)`, two launches.",
             "The timing method and the three figures are `tools/colour_cost.py`'s: *queued* is device time per call with the",
             "host off the critical path (%d calls enqueued behind several ms of other device work), *single* is HIP events" % CC.QUEUE,
             "around one call on an idle stream with the wrapper's checks inside the window, *host* is the host clock around",
             "the enqueue.  Medians of %d repetitions after %d warm-up calls.  *read* is the frame's bytes, read once." % (CC.REPS, CC.WARMUP), "",
             "| frame | coarse | input | read | queued | single | host |", "|---|---|---|---|---|---|---|"]
    for s in enc:
        for call, r in s["kernels"].items():
            lines.append("| %s | %s | %s | %.2f MB | %.1f µs | %.1f µs | %.1f µs |"
                         % (s["name"], s["coarse"], call, s["bytes"][call] / 1e6, r["queued"]["median"],
                            r["single"]["median"], r["host"]["median"]))
    lines += ["", "## `lsf_reloc_query`", "",
              "The 30 x 40 coarse image against random codes of %d ferns of %d decisions, one candidate, no harvest; three" % (FERNS, DECISIONS),
              "launches (the code, the distances, the selection).  *bandwidth* is the database's bytes over the queued time.",
              "",
              "| keyframes | database | queued | single | host | bandwidth |", "|---|---|---|---|---|---|"]
    for q in qry:
        c = q["call"]
        lines.append("| %d | %.3f MB | %.1f µs | %.1f µs | %.1f µs | %.1f GB/s |"
                     % (q["keyframes"], q["database_bytes"] / 1e6, c["queued"]["median"], c["single"]["median"],
                        c["host"]["median"], q["gb_per_s"]))
    w = frame["wall_ms"]
    lines += ["", "## A tracked and fused frame", "",
              "`SequenceFusion3d` at %d³, `tracking_reference=\"icp\"`, 640 x 480 (`tests/fusion_scene.py`): host clock around" % frame["n"],
              "`integrate()` and a device wait, frames k >= 1 of %d-frame sequences, %d repetitions after 2 warm-up ones, the two" % (frame["frames_per_sequence"], frame["reps"]),
              "sequences alternating.  *Without the keywords* is the code that did not change; *with relocaliser* is",
              "`relocaliser=fusion.Relocaliser()` (500 ferns, 30 x 40, 1024 keyframes; it implies `TrackingQuality()`): an encode,",
              "the verdict on records that are on the host already, and one harvesting query with its host copy of 48 bytes per",
              "fused frame.  Every frame of the run was tracked and fused.", "",
              "| sequence | median | p25 | p75 | frames |", "|---|---|---|---|---|"]
    for name, v in w.items():
        lines.append("| %s | %.3f ms | %.3f ms | %.3f ms | %d |" % (name, v["median"], v["p25"], v["p75"], v["count"]))
    lines += ["", ""]
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    stem = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "relocaliser_cost")
    os.makedirs(os.path.dirname(os.path.abspath(stem)), exist_ok=True)
    assert torch.cuda.is_available(), "the cost of the relocaliser is measured on the GPU"
    blocker = torch.zeros(CC.BLOCKER_FLOATS, dtype=torch.float32, device="cuda")
    enc = encodes(blocker)
    qry = queries(blocker)
    frame = frames()
    print(json.dumps(frame), flush=True)
    with open(stem + ".json", "w") as f:
        json.dump(dict(encode=enc, query=qry, frame=frame, warmup=CC.WARMUP, reps=CC.REPS, queue=CC.QUEUE), f, indent=1)
    write_md(stem + ".md", enc, qry, frame)


if __name__ == "__main__":
    main()
