"""Cost of the moving volume's brick store (profiles/volume_bricks_cost.md, .json), at 256^3 with and without the colour
volume, on a model that holds frame 0 of the sphere scene (tests/fusion_scene.py, tests/colour_scene.py), for a shift by
6 voxels on one axis and one by (32, 32, 32); the window sits at lattice origin (-3, 5, 13), so its faces cut bricks,
and with its low corner 40 voxels before the scene's centre, so that what leaves holds data.
1. The three entry points (device_volume_bricks.count, gather, scatter): the figures and the timing method are
   tools/colour_cost.py's (queued, single, host), the calls alternating within every repetition.
2. The stages of CanonicalVolume.shift(brick_store=) one by one, host clock around each with a device wait: count and the
   read of the total, gather, the rows' copy to the host, the store's merge, the upload of the rows, scatter, the
   store's clear.
3. The whole call out (everything is gathered) and back (everything is scattered), next to shift() alone in the same
   run, alternating, and next to the naive alternative: the leaving slabs copied densely to the host by torch slicing.
4. Bricks kept over bricks touched.
usage: volume_bricks_cost.py [OUT_STEM]"""
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
import levelsetfusion_python_amd as lsf  # noqa: E402
from levelsetfusion_python_amd import device_volume_bricks as B  # noqa: E402
from levelsetfusion_python_amd.device_volume_shift import retained_range  # noqa: E402

N = 256
SHIFTS = ((6, 0, 0), (32, 32, 32))
ORIGIN = (-3, 5, 13)
CORNER = N / 2 - 40  # voxels: the window's low faces pass 40 voxels before the scene's centre
WALL_WARMUP, WALL_REPS = 2, 9


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def walls(fns, prepare=None):
    """{name: stats of the wall time in ms}: the calls alternate within a repetition, `prepare` runs untimed before each"""
    raw = {name: [] for name in fns}
    for rep in range(WALL_WARMUP + WALL_REPS):
        for name in (list(fns) if rep % 2 == 0 else list(fns)[::-1]):
            state = prepare(name) if prepare else None
            ms, _ = wall_ms((lambda: fns[name](state)) if prepare else fns[name])
            if rep >= WALL_WARMUP:
                raw[name].append(ms)
    return {name: CC.stats(v) for name, v in raw.items()}


def model(colour):
    """a 256^3 model that holds frame 0, and the window's array_offset"""
    off = CC.offset(N) + CORNER  # the scene's centre lies near the window's low corner: what leaves there holds data
    vol = lsf.fusion.CanonicalVolume(N, colour=colour)
    if colour:
        d0, i0, _ = CS.frames()[0]
        vol.integrate_depth(d0, CC.CAM, S.true_twist(0), off, colour_image=i0)
    else:
        vol.integrate_depth(S.frames(1)[0], CC.CAM, S.true_twist(0), off)
    return vol, off


def fresh_store(colour, off):
    store = lsf.fusion.BrickStore(colour=colour)
    store.lattice_origin(off - np.array(ORIGIN, np.float64))  # the window sits at ORIGIN on the lattice
    return store


def leaving_slabs(shape, s):
    """the voxels that leave as at most three disjoint boxes of (z, y, x) slices: the x-slab over all y and z, the y-slab
    over the retained x, the z-slab over the retained x and y"""
    n = (shape[2], shape[1], shape[0])
    kept = [retained_range(m, max(-m, min(m, v))) for m, v in zip(n, s)]
    boxes = []
    for axis in range(3):
        k0, k1 = kept[axis]
        for a, b in ([(0, n[axis])] if k0 == k1 else [(0, k0), (k1, n[axis])]):
            box = [kept[j] if j < axis else (0, n[j]) for j in range(3)]
            box[axis] = (a, b)
            if all(q > p for p, q in box):
                boxes.append(tuple(slice(p, q) for p, q in box[::-1]))
        if k0 == k1:  # nothing is retained: the one box is the whole volume
            break
    return boxes


def one_case(colour, s, blocker):
    vol, off = model(colour)
    shape = vol.shape
    g = ORIGIN
    back = tuple(-v for v in s)
    pristine = (vol.tsdf.clone(), vol.weight.clone(), None if not colour else vol.colour.clone())

    def restore():
        vol.tsdf.copy_(pristine[0])
        vol.weight.copy_(pristine[1])
        if colour:
            vol.colour.copy_(pristine[2])

    # ---- the entry points -----------------------------------------------------------------------------------------------
    nb = int(np.prod(B.brick_grid(shape, g)[1]))
    flags, offsets = (torch.empty(nb, dtype=torch.int32, device="cuda") for _ in range(2))
    total = torch.empty(1, dtype=torch.int64, device="cuda")
    B.count(vol.weight, flags, offsets, total, g, s)
    k = int(total.item())
    new = lambda sh, dt: torch.empty(sh, dtype=dt, device="cuda")
    cube = (k, 8, 8, 8)
    rows = (new((k, 3), torch.int32), new(cube, torch.float32), new(cube, torch.float32),
            new(cube + (4,), torch.float32) if colour else None, new((k, 64), torch.uint8))
    B.gather(vol.tsdf, vol.weight, vol.colour, flags, offsets, k, *rows, g, s)
    coords_all = B.grid_coords(shape, g)
    touched = int(B.leaving_mask(shape, g, s, coords_all).reshape(nb, -1).any(axis=1).sum())
    # the way back: the window returns to g, and everything that left under s enters under -s
    dst = (torch.ones(shape, device="cuda"), torch.zeros(shape, device="cuda"),
           torch.zeros(shape + (4,), device="cuda") if colour else None)
    fns = {"count": lambda: B.count(vol.weight, flags, offsets, total, g, s),
           "gather": lambda: B.gather(vol.tsdf, vol.weight, vol.colour, flags, offsets, k, *rows, g, s),
           "scatter": lambda: B.scatter(*rows, *dst, g, back)}
    kernels = CC.measure(fns, blocker)
    row_bytes = k * (12 + 64 + 512 * (24 if colour else 8))

    # ---- the stages, host clock ---------------------------------------------------------------------------------------
    host_rows = tuple(None if t is None else t.cpu().numpy() for t in rows)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    taken = B.unpack_valid(host_rows[4])

    def merged_store(_=None):
        st = fresh_store(colour, off)
        st.merge(*host_rows)
        return st

    stages = walls({
        "count and the read of the total": lambda _: (B.count(vol.weight, flags, offsets, total, g, s), total.item()),
        "gather": lambda _: B.gather(vol.tsdf, vol.weight, vol.colour, flags, offsets, k, *rows, g, s),
        "rows to the host": lambda _: tuple(None if t is None else t.cpu().numpy() for t in rows),
        "merge": lambda st: st.merge(*host_rows),
        "lookup": lambda st: st.lookup_entering(*B.entering_flags(shape, g, back)),
        "upload": lambda _: tuple(up(a) for a in host_rows),
        "scatter": lambda _: B.scatter(*rows, *dst, g, back),
        "clear": lambda st: st.clear_valid(host_rows[0], taken),
    }, prepare=lambda name: (fresh_store(colour, off) if name == "merge" else
                             merged_store() if name in ("lookup", "clear") else None))

    # ---- the whole call ------------------------------------------------------------------------------------------------
    vol.shift((1, 0, 0), off)  # the spare buffers exist before a timed call
    restore()

    def prepared(name):
        restore()
        store = fresh_store(colour, off)
        if name == "shift(-s, brick_store=), all of it coming back":
            vol.shift(s, off, brick_store=store)
        return store

    slabs = leaving_slabs(shape, s)
    tensors = [vol.tsdf, vol.weight] + ([vol.colour] if colour else [])
    whole = walls({
        "shift(s) alone": lambda st: vol.shift(s, off),
        "shift(s, brick_store=), all of it leaving": lambda st: vol.shift(s, off, brick_store=st),
        "shift(-s, brick_store=), all of it coming back": lambda st: vol.shift(back, off + np.array(s, float),
                                                                               brick_store=st),
        "shift(s) and the leaving slabs copied densely": lambda st: (
            [t[box].contiguous().cpu() for t in (vol.tsdf, vol.weight) + ((vol.colour,) if colour else ())
             for box in slabs], vol.shift(s, off)),
    }, prepare=prepared)
    restore()
    store = fresh_store(colour, off)
    vol.shift(s, off, brick_store=store)
    last_out = dict(store.last)
    vol.shift(back, off + np.array(s, float), brick_store=store)
    last_back = dict(store.last)
    same = all(torch.equal(a.view(torch.int32)[pristine[1] != 0], b.view(torch.int32)[pristine[1] != 0])
               for a, b in zip((vol.tsdf, vol.weight), pristine[:2]))
    slab_bytes = int(sum(t[box].numel() * 4 for t in tensors for box in slabs))
    out = dict(n=N, colour=colour, shift=list(s), origin=list(g), grid_bricks=nb, bricks_touched=touched, bricks_kept=k,
               row_bytes=row_bytes, slab_bytes=slab_bytes, out=last_out, back=last_back,
               round_trip_restores_every_voxel_with_data=bool(same and len(store) == 0),
               kernels=kernels, stages_ms=stages, whole_ms=whole)
    del vol, pristine, rows, dst
    torch.cuda.empty_cache()
    return out


def write_md(path, cases):
    name = lambda c: "(%d, %d, %d)%s" % (*c["shift"], ", colour" if c["colour"] else "")
    lines = ["# Cost of the moving volume's brick store (MI355X)", "",
             "`tools/volume_bricks_cost.py` (raw numbers: `volume_bricks_cost.json`).  A %d³ model that holds frame 0 of the" % N,
             "sphere scene, the window at lattice origin (%d, %d, %d) so that its faces cut bricks and with its low corner" % ORIGIN,
             "%d voxels before the scene's centre so that what leaves holds data; nothing here had been measured before, so" % (N / 2 - CORNER),
             "no target was set in advance.", "",
             "## What leaves", "",
             "| shift | grid bricks | touched by what leaves | kept (hold data there) | kept / touched | voxels kept | "
             "rows | leaving slabs, dense |", "|---|---|---|---|---|---|---|---|"]
    for c in cases:
        lines.append("| %s | %d | %d | %d | %.2f | %d | %.2f MB | %.2f MB |"
                     % (name(c), c["grid_bricks"], c["bricks_touched"], c["bricks_kept"],
                        c["bricks_kept"] / max(c["bricks_touched"], 1), c["out"]["voxels_out"], c["row_bytes"] / 1e6,
                        c["slab_bytes"] / 1e6))
    lines += ["", "## The entry points", "",
              "The timing method and the three figures are `tools/colour_cost.py`'s: *queued* is device time per call with the",
              "host off the critical path (%d calls enqueued behind several ms of other device work), *single* is HIP events" % CC.QUEUE,
              "around one call on an idle stream with the wrapper's checks inside the window, *host* is the host clock around",
              "the enqueue.  Medians of %d repetitions after %d warm-up calls.  `count` is two launches (the flags, then the" % (CC.REPS, CC.WARMUP),
              "one-workgroup scan); `scatter` writes the gathered rows back into a window at the shifted origin.", "",
              "| shift | call | queued | single | host |", "|---|---|---|---|---|"]
    for c in cases:
        for call in ("count", "gather", "scatter"):
            r = c["kernels"][call]
            lines.append("| %s | %s | %.1f µs | %.1f µs | %.1f µs |" % (name(c), call, r["queued"]["median"],
                                                                         r["single"]["median"], r["host"]["median"]))
    lines += ["", "## The stages of `CanonicalVolume.shift(brick_store=)`", "",
              "Host clock around each stage with a device wait behind it, median of %d after %d warm-up calls: these" % (WALL_REPS, WALL_WARMUP),
              "include the launch and the wait, which the queued figures above leave out.", "",
              "| shift | " + " | ".join(cases[0]["stages_ms"]) + " |", "|---|" + "---|" * len(cases[0]["stages_ms"])]
    for c in cases:
        lines.append("| %s | " % name(c) + " | ".join("%.3f ms" % v["median"] for v in c["stages_ms"].values()) + " |")
    lines += ["", "## The whole call", "",
              "Host clock around the call and a device wait, the calls alternating within every repetition, each on a",
              "freshly restored model; `shift(s) alone` is the call without a store, whose code did not change.  The dense",
              "alternative copies the leaving slabs of every tensor to the host with torch slicing, then shifts.", "",
              "| shift | " + " | ".join(cases[0]["whole_ms"]) + " |", "|---|" + "---|" * len(cases[0]["whole_ms"])]
    for c in cases:
        lines.append("| %s | " % name(c) + " | ".join("%.2f ms" % v["median"] for v in c["whole_ms"].values()) + " |")
    lines += ["", "Every case's round trip (out, then back) restored every voxel with data bit for bit and left the store "
              "empty: %s." % ("yes" if all(c["round_trip_restores_every_voxel_with_data"] for c in cases) else "NO"), "", ""]
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    stem = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "volume_bricks_cost")
    os.makedirs(os.path.dirname(os.path.abspath(stem)), exist_ok=True)
    assert torch.cuda.is_available(), "the cost of the brick store is measured on the GPU"
    blocker = torch.zeros(CC.BLOCKER_FLOATS, dtype=torch.float32, device="cuda")
    cases = []
    for colour in (False, True):
        for s in SHIFTS:
            cases.append(one_case(colour, s, blocker))
            print(json.dumps(cases[-1]), flush=True)
    with open(stem + ".json", "w") as f:
        json.dump(dict(cases=cases, warmup=CC.WARMUP, reps=CC.REPS, queue=CC.QUEUE, wall_warmup=WALL_WARMUP,
                       wall_reps=WALL_REPS), f, indent=1)
    write_md(stem + ".md", cases)


if __name__ == "__main__":
    main()
