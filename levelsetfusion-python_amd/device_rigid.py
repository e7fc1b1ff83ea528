"""Torch-facing wrapper of the SDF-2-SDF rigid tracker's entry points (include/lsf_hip.h: lsf_rigid_gradient,
lsf_rigid_run).  The public drop-ins are rigid_opt/sdf_gradient_field.py and rigid_opt/sdf_2_sdf_optimizer2d.py."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import RigidParams, check, lib
from .device_core import require_gpu, stream_ptr
from .tsdf.generation import offsets_of, tsdf_params

RECORD = _lib.RIGID_RECORD_DOUBLES


def _field(x, name):
    if isinstance(x, torch.Tensor):
        t = (x if x.is_cuda else x.to("cuda")).to(torch.float32).contiguous()
    else:
        a = np.asarray(x)
        if a.dtype.kind not in "fiub":
            raise ValueError("%s must be numeric, got %s" % (name, a.dtype))
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda")
    if t.dim() != 2 or t.shape[0] < 2 or t.shape[1] < 2:
        raise ValueError("%s must be a 2-D field of at least 2 x 2, got shape %s" % (name, tuple(t.shape)))
    return t


def twist3(twist):
    t = np.asarray(twist, dtype=np.float64).reshape(-1)
    if t.size != 3:
        raise ValueError("twist must have 3 entries (t_x, t_z, theta), got %d" % t.size)
    return t


def gradient_wrt_twist(live_field, twist, array_offset, voxel_size=0.004):
    """(H, W, 3) float32 device tensor: calculate_gradient_wrt_twist of live_field (H, W) in one launch"""
    require_gpu()
    live = _field(live_field, "live_field")
    p = RigidParams()
    p.array_offset[:] = list(offsets_of(array_offset))
    p.voxel_size = float(voxel_size)
    if not p.voxel_size > 0.0:
        raise ValueError("voxel_size must be positive")
    p.twist[:] = list(twist3(twist))
    p.height, p.width = int(live.shape[0]), int(live.shape[1])
    out = torch.empty((p.height, p.width, 3), dtype=torch.float32, device="cuda")
    check(lib.lsf_rigid_gradient(ctypes.c_void_p(live.data_ptr()), ctypes.c_void_p(out.data_ptr()), ctypes.byref(p),
                                 stream_ptr()), "lsf_rigid_gradient")
    return out


def rigid_run(canonical, live_depth, depth_code, camera, image_y_coordinate, array_offset, iterations, rate, eta,
              voxel_size, generator_voxel_size, narrow_band_width_voxels, default_value=1, twist=None):
    """the whole optimize() enqueued: iterations + 1 launches and one copy back.  canonical: float32 device field
    (H, W); live_depth: device depth image (uint16 / float32 / float64, depth_code LSF_DEPTH_*).  Returns (final twist
    float64 (3,), records float64 (iterations, RIGID_RECORD_DOUBLES))."""
    require_gpu()
    canonical = _field(canonical, "canonical_field")
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError("iteration must be >= 0")
    P = np.asarray(camera.intrinsics.intrinsic_matrix)
    p = RigidParams()
    p.tsdf = tsdf_params(P, camera, live_depth, generator_voxel_size, narrow_band_width_voxels, image_y_coordinate,
                         default_value)
    p.array_offset[:] = list(offsets_of(array_offset))
    p.voxel_size = float(voxel_size)
    p.rate = float(rate)
    p.eta = float(np.float32(eta))
    p.depth_dtype = int(depth_code)
    p.height, p.width = int(canonical.shape[0]), int(canonical.shape[1])
    p.iterations = iterations
    # one buffer: [twist (3)][records (iterations x RECORD)] -- one copy back
    out = torch.zeros(3 + iterations * RECORD, dtype=torch.float64, device="cuda")
    if twist is not None:
        out[:3] = torch.from_numpy(twist3(twist))
    scratch = torch.empty(_lib.RIGID_SCRATCH_BYTES // 8, dtype=torch.float64, device="cuda")
    base = out.data_ptr()
    check(lib.lsf_rigid_run(ctypes.c_void_p(canonical.data_ptr()), ctypes.c_void_p(live_depth.data_ptr()),
                            ctypes.c_void_p(base), ctypes.c_void_p(base + 3 * 8), ctypes.c_void_p(scratch.data_ptr()),
                            ctypes.byref(p), stream_ptr()), "lsf_rigid_run")
    host = out.cpu().numpy()
    return host[:3].copy(), host[3:].reshape(iterations, RECORD).copy()
