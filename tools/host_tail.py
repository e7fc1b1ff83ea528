#!/usr/bin/env python3
"""host time around the two foreign calls of the default KillingFusion call (bench config 4: a 256^3 sphere pair, 50 fixed
iterations, the library-enqueued route lsf_state_run_begin / lsf_state_run_finish_rows), per step over a number of steps:

    entry    SlavchevaEngine.optimize entered -> lsf_state_run_begin called   (route, target, states, scratch, totals)
    between  lsf_state_run_begin returned -> lsf_state_run_finish_rows called (lists, records, result arrays, aftermath)
    tail     lsf_state_run_finish_rows returned -> SlavchevaEngine.optimize returned (the card idles until the next call)

and the whole drop-in step for scale.  Prints one JSON line: median, minimum and maximum in microseconds.
Usage: host_tail.py [size] [steps]"""
import gc
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import levelsetfusion_python_amd as lsf  # noqa: E402
from levelsetfusion_python_amd import _lib  # noqa: E402
from levelsetfusion_python_amd.engine_slavcheva import SlavchevaEngine  # noqa: E402
from levelsetfusion_python_amd.synthetic import sphere_pair  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
WARMUP = 10
BEGIN, FINISH = "lsf_state_run_begin", "lsf_state_run_finish_rows"
marks = {}


def timed(owner, name):
    fn = getattr(owner, name)

    def inner(*a, **k):
        t0 = time.perf_counter()
        try:
            return fn(*a, **k)
        finally:
            marks[name] = (t0, time.perf_counter())
    setattr(owner, name, inner)


for symbol in (BEGIN, FINISH):
    timed(_lib.lib, symbol)
timed(SlavchevaEngine, "optimize")

canonical, live0 = sphere_pair(n, 3, "cuda")
opt = lsf.SlavchevaOptimizer3d(field_size=n, compute_method=lsf.ComputeMethod.DIRECT, level_set_term_enabled=True,
                               smoothing_term_method=lsf.SmoothingTermMethod.KILLING,
                               maximum_warp_length_lower_threshold=0.0, max_iterations=50, min_iterations=50,
                               check_interval=50)
live = torch.empty_like(live0)
gc.collect()
gc.freeze()
gc.disable()
rows = dict(entry=[], between=[], tail=[], step=[])
for k in range(steps + WARMUP):
    live.copy_(live0)
    t0 = time.perf_counter()
    opt.optimize(live, canonical)
    t1 = time.perf_counter()
    if k < WARMUP:
        continue
    (e0, e1), (b0, b1), (f0, f1) = marks["optimize"], marks[BEGIN], marks[FINISH]
    rows["entry"].append(b0 - e0)
    rows["between"].append(f0 - b1)
    rows["tail"].append(e1 - f1)
    rows["step"].append(t1 - t0)
assert opt.engine.last_call.library_run and opt.engine.iteration_count == 50
print(json.dumps(dict(tool="host_tail", size=n, steps=steps,
                      us={name: dict(median=round(1e6 * statistics.median(v), 2), min=round(1e6 * min(v), 2),
                                     max=round(1e6 * max(v), 2)) for name, v in rows.items()})))
