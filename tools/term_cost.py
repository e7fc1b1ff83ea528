#!/usr/bin/env python3
"""Cost of the term-level kernel (lsf_term_gradient) on whole fields: Killing and data BASIC, planar device tensors,
gradient out with and without the float64 energy total.  Prints HIP-event times per call and the traffic model's
fraction of 8 TB/s (Killing: D warp planes in, D out; data BASIC: live, canonical, D caller-gradient planes in, D out).
Run it under  rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/term_cost.py  for per-dispatch times.
Usage: term_cost.py [reps]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from levelsetfusion_python_amd import _lib, device_core, device_terms  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50


def case(shape, term, energy):
    d = len(shape)
    g = torch.Generator(device="cuda").manual_seed(1)
    f = lambda k: torch.rand((k,) + shape, generator=g, device="cuda") * 0.2 - 0.1  # noqa: E731
    grid = device_core.make_grid(shape)
    n = device_core.n_voxels(grid)
    out = torch.empty((d,) + shape, device="cuda")
    total = torch.zeros(1, dtype=torch.float64, device="cuda") if energy else None
    if term == _lib.TERM_KILLING:
        warp = f(d)
        args = dict(warp=warp)
        bytes_ = 2 * d * 4 * n
    else:
        live, canonical, grads = f(1)[0], f(1)[0], f(d)
        args = dict(live=live, canonical=canonical, live_gradients=[grads[c] for c in range(d)])
        bytes_ = (2 + 2 * d) * 4 * n

    def run():
        device_terms.term_gradient(term, grid, gradient_out=out, energy_total=total, interleaved=False, **args)

    run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    name = "killing" if term == _lib.TERM_KILLING else "data_basic"
    print("%-10s %-12s energy=%d  %.4f ms  model %5.1f MB  %.2f TB/s = %.3f of 8 TB/s"
          % (name, "x".join(map(str, shape)), int(energy), ms, bytes_ / 1e6, bytes_ / ms / 1e9, bytes_ / ms / 1e9 / 8.0),
          flush=True)


for shape in ((512, 512), (256, 256, 256)):
    for term in (_lib.TERM_KILLING, _lib.TERM_DATA_BASIC):
        for energy in (False, True):
            case(shape, term, energy)
