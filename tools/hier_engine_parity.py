#!/usr/bin/env python
"""Everything a caller can observe of HierarchicalOptimizer2d / 3d over a fixed matrix of configurations, as ONE .npz --
the yardstick for changes to the host side of the hierarchical engine (engine_hier*.py) that must not change a bit:

    python tools/hier_engine_parity.py run OUT.npz            # on the commit before and on the commit after
    python tools/hier_engine_parity.py compare BEFORE.npz AFTER.npz [--unblocked-gradient]

Per case: the warp, per-level iteration counts, maxima, arg-max, data and Tikhonov energies, engine.last_gradient (and
whether it is None), last_call.blocked_levels and, where switched on, the convergence reports' numbers, iteration_data
and what the iteration hook was handed.  The matrix: D = 2 and 3; Tikhonov term on / off; no gradient kernel, 3 and 7
taps; blocked_levels, use_graphs, fused_filter, defer_maximum on and off; a threshold of 0 and one that fires inside a
batch / a graph replay / a blocked launch; iteration limits 0, 1, 3 and ones that are and are not multiples of the batch;
energies, reports, telemetry, a hook; linear resampling; a 3-D pyramid whose finest level has 2^23 voxels
(lsf_convolve_xyz) over levels that have fewer.  Only the public optimizers are used.

compare demands np.array_equal (NaNs equal) of every array (the energies and the reports' statistics: see compare).
--unblocked-gradient: for the cases with neither Tikhonov
term nor gradient kernel on blocked levels, AFTER's last_gradient is held against BEFORE's value of the same case with
blocked_levels off (the one place where the blocked driver used to leave another engine state than the per-iteration one)."""
import contextlib
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

BATCH = 8  # check_interval of every case: the eager batch, the graph's K and (Tikhonov only) the blocked launch


def cases():
    """(name, dims, shape, constructor keywords, extras) -- extras: stop_at (the threshold is put just above the first
    maximum from that iteration on that is below every earlier one, on level stop_level of an unterminated run: that
    level then ends there), reports / telemetry / hook / energy"""
    out = []

    def add(dims, shape, tik, taps, it, stop_at=None, chunk=8, linear=False, stop_level=0, **more):
        flags = {k: more.pop(k) for k in ("reports", "telemetry", "hook", "energy") if k in more}
        if flags.get("hook") and not tik and not taps:
            flags["reports"] = True  # (with neither term a level keeps a gradient to hand out only for the reports)
        name = "D%d,%s,tik=%d,taps=%d,it=%d,stop=%s@%d,lin=%d,%s" % (
            dims, "x".join(map(str, shape)), tik, taps, it, stop_at, stop_level, linear,
            ",".join("%s=%d" % (k[:7], v) for k, v in sorted(more.items())))
        if flags:
            name += "," + "+".join(sorted(k for k, v in flags.items() if v))
        kw = dict(tikhonov_term_enabled=bool(tik), gradient_kernel_enabled=bool(taps), maximum_chunk_size=chunk, rate=0.1,
                  maximum_iteration_count=it, tikhonov_strength=0.05, check_interval=BATCH)
        out.append((name, dims, tuple(shape), kw, dict(taps=taps, stop_at=stop_at, stop_level=stop_level, linear=linear,
                                                       options=more, **flags)))

    for tik in (1, 0):
        for taps in (0, 3, 7):
            # 2-D, four levels 16^2 .. 128^2
            for blocked, graphs in ((1, 1), (0, 1), (0, 0)):
                opts = dict(blocked_levels=blocked, use_graphs=graphs)
                for it in (0, 1, 3, 13, 16, 20):
                    add(2, (128, 128), tik, taps, it, **opts)
                for it, stop_at in ((20, 10), (13, 4), (16, 7)):
                    for stop_level in (0, -1):
                        add(2, (128, 128), tik, taps, it, stop_at, stop_level=stop_level, **opts)
            for extra in ("reports", "telemetry", "hook", "energy"):
                for stop_at in (None, 5):
                    for blocked, graphs in ((1, 1), (0, 1), (0, 0)):
                        add(2, (128, 128), tik, taps, 11, stop_at, blocked_levels=blocked, use_graphs=graphs, **{extra: True})
            # 3-D, four levels 8^3 .. 64^3 (graph replay by default; the x and y passes in one launch from nx % 4 == 0)
            for graphs, fused, defer in ((1, 1, 1), (0, 1, 1), (0, 0, 1), (0, 1, 0), (1, 1, 0)):
                opts = dict(use_graphs=graphs, fused_filter=fused, defer_maximum=defer)
                for it in (0, 1, 3, 13):
                    add(3, (64, 64, 64), tik, taps, it, **opts)
                add(3, (64, 64, 64), tik, taps, 13, 5, **opts)
            add(3, (32, 32, 32), tik, taps, 9, chunk=4, linear=True)
            add(3, (32, 32, 32), tik, taps, 9, 4, chunk=4, linear=True, use_graphs=0)
            for extra in ("reports", "telemetry", "hook", "energy"):
                add(3, (32, 32, 32), tik, taps, 6, chunk=4, **{extra: True})
                add(3, (32, 32, 32), tik, taps, 6, 2, chunk=4, **{extra: True})
    # finest level 128 x 256 x 256 = 2^23 voxels: lsf_convolve_xyz there, graph replay and pass-by-pass filters below it
    for tik, taps, fused, defer, stop_at in ((1, 7, 1, 1, None), (1, 7, 1, 0, None), (1, 7, 0, 1, None), (1, 3, 1, 1, 3),
                                             (0, 7, 1, 1, None), (1, 0, 1, 1, None)):
        add(3, (128, 256, 256), tik, taps, 6, stop_at, fused_filter=fused, defer_maximum=defer)
    return out


def _fields(dims, shape):
    from levelsetfusion_python_amd.synthetic import sphere_pair
    n = max(shape)
    canonical, live = sphere_pair(n, dims, "cuda")
    lo = [(n - s) // 2 for s in shape]
    cut = tuple(slice(a, a + s) for a, s in zip(lo, shape))
    return canonical[cut].contiguous(), live[cut].contiguous()


def _optimizer(lsf, dims, kw, extras, threshold):
    cls = lsf.HierarchicalOptimizer2d if dims == 2 else lsf.HierarchicalOptimizer3d
    more = {}
    if extras["linear"]:
        more["resampling_strategy"] = cls.ResamplingStrategy.LINEAR
    if extras.get("energy"):
        more["verbosity_parameters"] = cls.VerbosityParameters(print_iteration_data_energy=True,
                                                               print_iteration_tikhonov_energy=True)
    more["logging_parameters"] = cls.LoggingParameters(
        collect_per_level_convergence_reports=bool(extras.get("reports")),
        collect_per_level_iteration_data=bool(extras.get("telemetry")))
    kernel = lsf.generate_1d_sobolev_kernel(extras["taps"], 0.1) if extras["taps"] else None
    return cls(kernel=kernel, maximum_warp_update_threshold=threshold, engine_options=extras["options"], **more, **kw)


def run_case(lsf, dims, shape, kw, extras):
    canonical, live = _fields(dims, shape)
    threshold = 0.0
    if extras["stop_at"] is not None:
        free = _optimizer(lsf, dims, kw, dict(extras, reports=False, telemetry=False, hook=False, energy=False), 0.0)
        free.optimize(canonical, live)
        maxima = np.float32(free.get_per_level_maximum_updates()[extras["stop_level"]])
        lowest = np.minimum.accumulate(maxima)
        new_low = [j for j in range(1, len(maxima)) if maxima[j] < lowest[j - 1]]
        at = next((j for j in new_low if j >= extras["stop_at"]), new_low[-1] if new_low else 0)
        threshold = float(np.nextafter(maxima[at], np.float32(np.inf)))
    opt = _optimizer(lsf, dims, kw, extras, threshold)
    handed = []
    if extras.get("hook"):
        opt.iteration_hook = lambda level, it, warp, g, m: handed.append((level, it, warp.cpu().numpy(), g.cpu().numpy(), m))
    with contextlib.redirect_stdout(io.StringIO()):
        warp = opt.optimize(canonical, live)
    eng = opt.engine
    res = eng.level_results
    cat = lambda rows, dtype: np.concatenate([np.asarray(r, dtype=dtype).reshape(-1) for r in rows] or [np.zeros(0, dtype)])
    g = eng.last_gradient
    out = dict(
        warp=warp.cpu().numpy(), threshold=np.float64(threshold),
        counts=np.array([r.iteration_count for r in res], np.int64),
        limit_reached=np.array([r.iteration_limit_reached for r in res], np.bool_),
        voxel_counts=np.array([r.voxel_count for r in res], np.int64),
        maxima=cat([r.max_updates for r in res], np.float32), argmax=cat([r.argmax for r in res], np.int64),
        data_energies=cat([r.data_energies for r in res], np.float64),
        tikhonov_energies=cat([r.tikhonov_energies for r in res], np.float64),
        last_gradient_is_none=np.array(g is None), last_gradient=np.zeros(0, np.float32) if g is None else g.cpu().numpy(),
        blocked_levels=np.array(eng.last_call.blocked_levels, np.int64))
    if extras.get("reports"):
        rows = []
        for r in opt.get_per_level_convergence_reports():
            w, t = r.warp_delta_statistics, r.tsdf_difference_statistics
            rows.append([r.iteration_count, r.iteration_limit_reached, w.ratio_above_min_threshold, w.length_min, w.length_max,
                         w.length_mean, w.length_standard_deviation, *(list(w.longest_warp_location) + [0])[:3],
                         w.is_largest_below_min_threshold, w.is_largest_above_max_threshold, t.difference_min,
                         t.difference_max, t.difference_mean, t.difference_standard_deviation,
                         *(list(t.biggest_difference_location) + [0])[:3]])
        out["reports"] = np.array(rows, np.float64)
    if extras.get("telemetry"):
        levels = eng.iteration_data
        out["telemetry_counts"] = np.array([len(level) for level in levels], np.int64)
        for k, what in enumerate(("warp", "data", "tikhonov")):
            out["telemetry_" + what] = cat([s[k].cpu().numpy() for level in levels for s in level if s[k] is not None],
                                           np.float32)
    if extras.get("hook"):
        out["hook_calls"] = np.array([(h[0], h[1]) for h in handed], np.int64).reshape(-1, 2)
        out["hook_maxima"] = np.array([h[4] for h in handed], np.float64)
        out["hook_warps"] = cat([h[2] for h in handed], np.float32)
        out["hook_gradients"] = cat([h[3] for h in handed], np.float32)
    return out


def run(path):
    import levelsetfusion_python_amd as lsf
    arrays = {}
    matrix = cases()
    assert len({c[0] for c in matrix}) == len(matrix), "case names must be unique"
    for name, dims, shape, kw, extras in matrix:
        got = run_case(lsf, dims, shape, kw, extras)
        print("%-110s counts %s blocked %d" % (name, got["counts"].tolist(), int(got["blocked_levels"])), flush=True)
        for key, value in got.items():
            arrays[name + "/" + key] = value
    np.savez(path, **arrays)
    print("%d cases, %d arrays -> %s" % (len(matrix), len(arrays), path))


SUMMED = ("data_energies", "tikhonov_energies", "reports")  # float64 sums accumulated with atomics, in arrival order


def compare(before, after, unblocked_gradient):
    """every array equal -- except that the atomically summed ones, which a commit does not reproduce bit for bit against
    ITSELF (compare two runs of one commit to see it), may differ by the rounding of a reordered float64 sum: 1e-9
    relative, a million times what 2^14 .. 2^23 addends of one sign reorder to and a million times less than any change
    of what is summed"""
    a, b = np.load(before), np.load(after)
    if sorted(a.files) != sorted(b.files):
        print("the two files do not hold the same arrays")
        return 1
    bad, reordered, redirected = {}, {}, 0
    for key in a.files:
        want = key
        case, what = key.rsplit("/", 1)
        if (unblocked_gradient and what in ("last_gradient", "last_gradient_is_none") and "tik=0,taps=0," in case
                and int(a[case + "/blocked_levels"]) > 0):
            want = case.replace("blocked=1", "blocked=0") + "/" + what  # (a KeyError: the matrix lost the twin)
            redirected += 1
        x, y = a[want], b[key]
        if x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == "f"):
            continue
        if what in SUMMED and x.shape == y.shape and np.allclose(x, y, rtol=1e-9, atol=0.0, equal_nan=True):
            reordered[what] = reordered.get(what, 0) + 1
        else:
            bad.setdefault(what, []).append(key)
    print("%d arrays compared (%d of them last_gradient against the unblocked run): %d differ, %d more only by the order of an "
          "atomic sum %r" % (len(a.files), redirected, sum(map(len, bad.values())), sum(reordered.values()), reordered))
    for what, keys in bad.items():
        print("  DIFFERS: %d x %s, e.g. %s" % (len(keys), what, keys[0]))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3], "--unblocked-gradient" in sys.argv[4:]))
    else:
        sys.exit(__doc__)
