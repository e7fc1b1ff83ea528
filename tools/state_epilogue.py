"""What the END of an INTERIOR list-walk launch costs (needs the -DLSF_STATE_TRACE build: tools/build_variant.sh trace -
-DLSF_STATE_TRACE): per traced launch, over its workgroups, the epilogue (last wave of the workgroup out of the loop ->
the workgroup's last stamp behind block_reduce_commit) and the drain (first wave out of the loop -> last wave out of the
loop), from the 100 MHz stamps wave_row[2] / wave_row[3].  usage: state_epilogue.py [size] [launches]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("LSF_HIP_LIBRARY", os.path.join(ROOT, "levelsetfusion-python_amd/lib/variants/trace.so"))
sys.path.insert(0, ROOT)
import ctypes
import numpy as np
import torch
import levelsetfusion_python_amd as lsf
from levelsetfusion_python_amd import _lib, device as dev
from levelsetfusion_python_amd.synthetic import sphere_pair

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 6
eng = lsf.SlavchevaOptimizer3d(field_size=n, compute_method=lsf.ComputeMethod.DIRECT, level_set_term_enabled=True,
                               smoothing_term_method=lsf.SmoothingTermMethod.KILLING).engine
grid = dev.make_grid((n, n, n))
c, l = sphere_pair(n, 3, "cuda")
bands = dev.band_lists(l, c, grid)
rec = dev.new_records(1, "cuda")
st = dev.state_pack(l, None, grid, copies=2)
fn = _lib.lib.lsf_debug_set_state_trace
fn.restype = ctypes.c_int
fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
waves = torch.zeros(4096 * 16 * 8, dtype=torch.int64, device="cuda")
for i in range(6):  # warm-up, untraced
    dev.slavcheva_state_iteration(st[i % 2], c, st[(i + 1) % 2], grid, eng.params, None, rec, 0, bands[0])
torch.cuda.synchronize()
assert fn(ctypes.c_void_p(0), ctypes.c_void_p(waves.data_ptr())) == 0
print("%d^3 sphere pair, INTERIOR list of %d voxels; times in us (stamps tick at 100 MHz: 0.01 us)" % (n, bands[0].count))
print("launch  workgroups | epilogue: median  mean   max  slowest-CU | drain: median  mean   max  slowest-CU | span")
ep_all, dr_all, slow_all = [], [], []
for k in range(launches):
    waves.zero_()
    # three launches back to back as in a call; the stamps of the last one are what is read
    for i in range(3):
        dev.slavcheva_state_iteration(st[i % 2], c, st[(i + 1) % 2], grid, eng.params, None, rec, 0, bands[0])
    torch.cuda.synchronize()
    wv = waves.cpu().numpy().reshape(4096, 16, 8)
    wv = wv[: int((wv[:, 0, 0] != 0).sum())]
    out_of_loop, behind_commit = wv[..., 2] * 0.01, wv[..., 3] * 0.01
    epilogue = behind_commit.max(axis=1) - out_of_loop.max(axis=1)
    drain = out_of_loop.max(axis=1) - out_of_loop.min(axis=1)
    slowest = int(behind_commit.max(axis=1).argmax())  # the workgroup (= CU) whose last wave ends the launch
    span = behind_commit.max() - wv[..., 0].min() * 0.01
    print("%6d  %10d | %16.2f %5.2f %5.2f %11.2f | %13.2f %5.2f %5.2f %11.2f | %5.2f" % (
        k, len(wv), np.median(epilogue), epilogue.mean(), epilogue.max(), epilogue[slowest], np.median(drain), drain.mean(),
        drain.max(), drain[slowest], span))
    ep_all.append(np.median(epilogue)); dr_all.append(np.median(drain)); slow_all.append(epilogue[slowest])
assert fn(ctypes.c_void_p(0), ctypes.c_void_p(0)) == 0
print("over %d launches: epilogue median %.2f us (slowest CU: median %.2f), drain median %.2f us" % (
    launches, float(np.median(ep_all)), float(np.median(slow_all)), float(np.median(dr_all))))
