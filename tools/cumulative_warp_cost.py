"""Cost of the cumulative warp (profiles/cumulative_warp_cost.md, .json): SlavchevaOptimizer3d in bench.py's KillingFusion
configuration on bench.py's sphere pair (256^3, 50 fixed iterations), three ways in one run:
  keyword_on            cumulative_warp=True: the general path plus one composition launch per iteration and band list
  launch_by_launch_off  engine_options=dict(library_run=False), keyword off: the same path without the added launches --
                        the baseline the added launches are counted against
  library_run_off       the default library-enqueued call, keyword off
Host clock around STEPS calls (each preceded by the copy of a fresh live field, as bench.py's step is) between device
synchronisations, the three alternating over ROUNDS rounds after WARMUP calls each, cyclic GC parked as in bench.py.
Then lsf_cumulative_warp_compose alone: HIP events around REPS back-to-back launches over the call's own band lists on a
state of the call's final fields, ping-pong between two PSI buffers, against 48 B per listed voxel at 8 TB/s.
usage: cumulative_warp_cost.py [OUT_JSON]      cumulative_warp_cost.py --trace CALLS   (keyword-on calls only, for a
kernel trace taken in a run of its own: rocprofv3 --kernel-trace --stats -- python tools/cumulative_warp_cost.py --trace 6)"""
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import levelsetfusion_python_amd as lsf  # noqa: E402
from levelsetfusion_python_amd import device as dev  # noqa: E402
from levelsetfusion_python_amd.synthetic import sphere_pair  # noqa: E402

N, ITERATIONS, WARMUP, STEPS, ROUNDS, REPS = 256, 50, 5, 20, 4, 200


def optimizer(**kw):
    return lsf.SlavchevaOptimizer3d(out_path=None, field_size=N, compute_method=lsf.ComputeMethod.DIRECT,
                                    level_set_term_enabled=True, smoothing_term_method=lsf.SmoothingTermMethod.KILLING,
                                    gradient_descent_rate=0.1, data_term_weight=1.0, smoothing_term_weight=0.2,
                                    isomorphic_enforcement_factor=0.1, level_set_term_weight=0.2,
                                    maximum_warp_length_lower_threshold=0.0, max_iterations=ITERATIONS,
                                    min_iterations=ITERATIONS, check_interval=ITERATIONS, **kw)


def main():
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    device = torch.device("cuda:0")
    canonical, live0 = sphere_pair(N, 3, device)
    live = torch.empty_like(live0)

    def step(opt):
        live.copy_(live0)  # a fresh pair every step (optimize() warps live in place)
        opt.optimize(live, canonical)
        return len(opt.log.max_warps)

    if len(sys.argv) > 2 and sys.argv[1] == "--trace":
        opt = optimizer(cumulative_warp=True)
        for _ in range(int(sys.argv[2])):
            assert step(opt) == ITERATIONS
        torch.cuda.synchronize()
        return
    variants = {"keyword_on": optimizer(cumulative_warp=True),
                "launch_by_launch_off": optimizer(engine_options=dict(library_run=False)),
                "library_run_off": optimizer()}
    for opt in variants.values():
        for _ in range(WARMUP):
            assert step(opt) == ITERATIONS
    assert [o.engine.last_call.library_run for o in variants.values()] == [False, False, True]
    gc.collect()
    gc.freeze()
    gc.disable()
    times = {name: [] for name in variants}
    for _ in range(ROUNDS):
        for name, opt in variants.items():
            step(opt)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(STEPS):
                step(opt)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / STEPS * 1e3)
    gc.enable()

    # the composition kernel alone, over the call's own band lists
    on = variants["keyword_on"]
    step(on)
    eng = on.engine
    bands, grid = eng._fast.bands, eng._fast.grid
    listed = sum(b.count for b in bands)
    state = dev.state_pack(live, dev.deinterleave(on.warp_field.contiguous(), 3), grid, copies=1)[0]
    psi = [torch.zeros_like(state), torch.zeros_like(state)]

    def compose(k):
        for b in bands:
            if b.count:
                dev.cumulative_warp_compose(state, psi[k % 2], psi[(k + 1) % 2], grid, None, b)

    for k in range(4):
        compose(k)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(REPS):
        compose(k)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / REPS * 1e3
    out = {"size": N, "iterations": ITERATIONS, "warmup": WARMUP, "steps_per_round": STEPS, "ms_per_call_by_round": times,
           "band_lists": [dict(subset=b.subset, count=b.count) for b in bands], "listed_voxels": listed,
           "sparse_states": bool(eng.last_call.sparse_states), "compose_reps": REPS,
           "compose_us_per_iteration": us, "compose_bytes_per_iteration": 48 * listed,
           "compose_floor_us_at_8_TB_per_s": 48.0 * listed / 8e12 * 1e6,
           "compose_TB_per_s": 48.0 * listed / (us * 1e-6) / 1e12}
    print(json.dumps(out, indent=1))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
